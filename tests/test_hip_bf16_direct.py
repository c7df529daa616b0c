"""The bf16-operand direct convolution kernels (csrc/igemm.hip: igemm_kernel<.., BF16>, igemm_multi_kernel<.., true>,
pgemm_kernel<.., BF16>, wgrad_bf16_kernel), one route per case (tests/conv_cases.py: B16_CASES), on run_case of
tests/test_hip_direct_conv.py.

Every case runs its launch under set_precision("bf16"), asserts from the launch records that exactly the expected kernel ran --
the four launchers write four distinct (kind 3, cfg) records -- and then faces the two references of tests/conv_oracle.py:
  - exact: integers of {-3 ... 3} are bf16 numbers, so the result must equal the fp64 reference bit for bit;
  - real: the kernels round the two MFMA operands to bf16 (nearest, ties to even) when they stage them and keep everything else
    fp32, so they compute an fp32 evaluation of the convolution of the ROUNDED operands: the fp32 a-priori bound, unchanged,
    around the oracle on operands rounded by conv_oracle.bf16_rne.  tests/test_conv_oracle_cpu.py shows that a kernel that stayed
    fp32, and one that truncates, both leave that bound.
The cases named b16_keeps_* must NOT change: bf16 mode leaves them on their fp32 kernel, with the fp32 record and the unrounded
reference."""
import time

import pytest

from tests import conv_cases as CC
from tests.test_hip_direct_conv import dev, run_case  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CC.B16_CASES, ids=[c.id for c in CC.B16_CASES])
def test_bf16_direct_conv(dev, case, tmp_path):
    t0 = time.perf_counter()
    run_case(case, dev, tmp_path / "launches.csv")
    print(f"CASE_SECONDS {case.id} {time.perf_counter() - t0:.2f}")
