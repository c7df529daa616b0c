"""The eager half of the prepared-weight cache (tg_hip.ops: _wprep, _wstamp, _prepared, weights_updated, _prepare_batch), one
transition per test: a torch in-place write (version bump), a `.data` write with and without weights_updated (the out-of-band
stamp, WPREP_VERIFY), one weight under several keys (two spatial sizes, both modes), an entry the batched refresh skips because
it was not used, a precision switch (the precision is part of the key) and a weight address the allocator hands out again.

Every convolution result is held against two references: (a) the same call with WPREP_CACHE off, bit for bit -- the cache adds
nothing; (b) a float64 CPU conv2d / conv_transpose2d of the weights AS THEY ARE NOW with tests/test_hip_ops.py's `close` and
the tolerances its conv test uses (fwd: defaults, dgrad: rtol 2e-4) -- a fault common to both paths cannot hide.  A stale
prepared buffer misses both: the updates below move every weight by far more than the tolerance, which each test asserts on the
references themselves.  Each test first asserts that its geometry and mode HAVE a prepared form (tg_conv_wprep_bytes > 0) and,
where it leans on the batched refresh, that the entry is batchable.  All tests run with WPREP_BATCH on and off."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_ops import close

pytestmark = pytest.mark.gpu

S3 = (32, 64, 3, 1, 1)            # Cin, Cout, k, stride, pad: a stride-1 3x3 layer.  Forward: the Winograd F(2x2,3x3) transform;
                                  # dgrad (N = Cin = 32 is no Winograd launch): the transposed weights.  Both are prepared forms.
S3_A, S3_B = (2, 17, 19), (2, 24, 40)          # B, H, W: tests/wino_cases.py's odd geometry and a second size of the same layer
S4 = (64, 8, 4, 2, 1)             # the 4x4 stride-2 layer of tests/wino_cases.py's w22 dgrad cases (F(2x2,2x2))
S4_A = (2, 36, 44)
DGRAD_RTOL = 2e-4                 # tests/test_hip_ops.py::test_conv_fwd_dgrad_wgrad


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(params=[True, False], ids=["batch", "nobatch"])
def batch(request, monkeypatch):
    from tg_hip import ops as O
    monkeypatch.setattr(O, "WPREP_BATCH", request.param)
    monkeypatch.setattr(O, "WPREP_CACHE", True)
    monkeypatch.setattr(O, "WPREP_VERIFY", False)
    return request.param


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class Layer:
    """One conv weight on the device (channels_last, as the models store it) and its inputs at the sizes a test asks for."""

    def __init__(self, dev, spec, seed):
        self.dev, self.spec = dev, spec
        self.cin, self.cout, self.k, self.s, self.p = spec
        self.gen = torch.Generator().manual_seed(seed)
        self.w = self.new_weight()
        self.bias = (torch.randn(self.cout, generator=self.gen) * 0.1).to(dev)
        self.io = {}

    def new_weight(self):
        w = torch.randn(self.cout, self.cin, self.k, self.k, generator=self.gen) * 0.1
        return w.contiguous(memory_format=torch.channels_last).to(self.dev)

    def out_hw(self, H, W):
        return (H + 2 * self.p - self.k) // self.s + 1, (W + 2 * self.p - self.k) // self.s + 1

    def inputs(self, bhw):
        if bhw not in self.io:
            B, H, W = bhw
            Ho, Wo = self.out_hw(H, W)
            self.io[bhw] = (torch.randn(B, H, W, self.cin, generator=self.gen).to(self.dev),
                            torch.randn(B, Ho, Wo, self.cout, generator=self.gen).to(self.dev))
        return self.io[bhw]

    def geom(self, bhw):
        from tg_hip import lib as L
        from tg_hip import ops as O
        B, H, W = bhw
        Ho, Wo = self.out_hw(H, W)
        return L.TgConv(B, H, W, self.cin, Ho, Wo, self.cout, self.k, self.s, self.p, O._precision)

    def prepared_bytes(self, bhw, mode):
        from tg_hip import lib as L
        return L.load().tg_conv_wprep_bytes(C.byref(self.geom(bhw)), mode)

    def entry(self, bhw, mode):
        from tg_hip import ops as O
        g = self.geom(bhw)
        return O._wprep.get((O.weight_view(self.w).data_ptr(), mode, g.H, g.W, g.Cin, g.Cout, g.k, g.stride, g.pad, g.precision))

    def run(self, bhw, mode):
        from tg_hip import ops as O
        x, dy = self.inputs(bhw)
        if mode == O.WPREP_FWD:
            return O.conv_fwd(x, self.w, self.bias, self.k, self.s, self.p)
        return O.conv_dgrad(dy, self.w, tuple(x.shape), self.k, self.s, self.p)

    def ref64(self, bhw, mode):
        """float64 on the CPU, from the weights as they are on the device now; NHWC."""
        from tg_hip import ops as O
        x, dy = self.inputs(bhw)
        w = self.w.detach().double().cpu()
        if mode == O.WPREP_FWD:
            return nhwc(F.conv2d(nchw(x.double().cpu()), w, self.bias.double().cpu(), self.s, self.p))
        return nhwc(F.conv_transpose2d(nchw(dy.double().cpu()), w, None, self.s, self.p))

    def require_prepared(self, uses):
        for bhw, mode in uses:
            assert self.prepared_bytes(bhw, mode) > 0, f"{self.spec} at {bhw}, mode {mode}: no prepared form -- the test would be vacuous"

    def check(self, uses, what):
        """Every (size, mode) of `uses` through the cache, against the cache-off call (bits) and float64 (close).  Returns the
        float64 references."""
        from tg_hip import ops as O
        refs = []
        for bhw, mode in uses:
            assert O.WPREP_CACHE
            y = self.run(bhw, mode)
            O.WPREP_CACHE = False
            try:
                y0 = self.run(bhw, mode)
            finally:
                O.WPREP_CACHE = True
            bad = int((y.view(torch.int32) != y0.view(torch.int32)).sum())
            assert bad == 0, f"{what}: {self.spec} at {bhw}, mode {mode}: {bad} of {y.numel()} elements differ from the cache-off call"
            ref = self.ref64(bhw, mode)
            if mode == O.WPREP_FWD:
                close(y, ref)
            else:
                close(y, ref, rtol=DGRAD_RTOL)
            refs.append(ref)
        return refs


def moved(before, after):
    """The update changed every reference by far more than `close` allows: a result from the old weights cannot pass."""
    for a, b in zip(before, after):
        assert float((a - b).abs().max()) > 100 * (1e-5 + DGRAD_RTOL * float(b.abs().max()))


def uses_s3():
    from tg_hip import ops as O
    return [(S3_A, O.WPREP_FWD), (S3_B, O.WPREP_FWD), (S3_A, O.WPREP_DGRAD)]


def uses_s4():
    from tg_hip import ops as O
    return [(S4_A, O.WPREP_DGRAD)]


def layers(dev, seed):
    out = []
    for spec, uses in ((S3, uses_s3()), (S4, uses_s4())):
        layer = Layer(dev, spec, seed + len(out))
        layer.require_prepared(uses)
        out.append((layer, uses))
    return out


def test_torch_inplace_write_is_seen(dev, batch):
    """forward, w.mul_(1.5) under no_grad (torch bumps _version), forward."""
    for layer, uses in layers(dev, 100):
        r0 = layer.check(uses, "first use")
        v0 = layer.w._version
        with torch.no_grad():
            layer.w.mul_(1.5)
        assert layer.w._version > v0
        moved(r0, layer.check(uses, "after w.mul_"))


def test_data_write_with_weights_updated_is_seen(dev, batch):
    """forward and dgrad, w.data.add_ (no version bump: only the out-of-band stamp can tell), weights_updated, forward and dgrad."""
    from tg_hip import ops as O
    for layer, uses in layers(dev, 200):
        r0 = layer.check(uses, "first use")
        v0 = layer.w._version
        layer.w.data.add_(0.25)
        assert layer.w._version == v0, "a .data write is expected to be invisible to torch's version counter"
        if batch:
            for bhw, mode in uses:
                ent = layer.entry(bhw, mode)
                assert ent is not None and ent[3] and ent[4], "the entry is expected to go through the batched refresh"
        O.weights_updated([layer.w])
        if batch:
            for bhw, mode in uses:
                assert layer.entry(bhw, mode)[4] is False          # the batch took it
        moved(r0, layer.check(uses, "after .data write + weights_updated"))


def test_verify_raises_on_a_data_write_without_weights_updated(dev, batch, monkeypatch):
    from tg_hip import lib as L
    from tg_hip import ops as O
    monkeypatch.setattr(O, "WPREP_VERIFY", True)
    for layer, uses in layers(dev, 300):
        for bhw, mode in uses:
            layer.run(bhw, mode)
            layer.run(bhw, mode)                     # a hit on a fresh entry: verified, no raise
        layer.w.data.mul_(2.0)
        for bhw, mode in uses:
            with pytest.raises(L.TgError, match="stale"):
                layer.run(bhw, mode)
        torch.cuda.synchronize()


def test_verify_passes_on_a_fresh_cache(dev, batch, monkeypatch):
    from tg_hip import ops as O
    monkeypatch.setattr(O, "WPREP_VERIFY", True)
    for layer, uses in layers(dev, 400):
        r0 = layer.check(uses, "first use")
        layer.check(uses, "second use (hits, verified)")
        layer.w.data.add_(0.25)
        O.weights_updated([layer.w])
        moved(r0, layer.check(uses, "after a reported update (verified)"))


def test_one_weight_under_several_keys(dev, batch):
    """Forward at two spatial sizes and dgrad at one hold three entries of one weight; one update reaches all three."""
    from tg_hip import ops as O
    layer = Layer(dev, S3, 500)
    uses = uses_s3()
    layer.require_prepared(uses)
    r0 = layer.check(uses, "first use")
    ents = [layer.entry(bhw, mode) for bhw, mode in uses]
    assert all(e is not None for e in ents) and len({id(e) for e in ents}) == 3
    assert len({e[2].data_ptr() for e in ents}) == 3
    layer.w.data.mul_(-0.5)
    O.weights_updated([layer.w])
    r1 = layer.check(uses, "after the update")
    moved(r0, r1)
    with torch.no_grad():
        layer.w.add_(0.125)
    moved(r1, layer.check(uses, "after an in-place write on top"))


def test_entry_unused_across_two_updates(dev, batch):
    """The batched refresh skips entries not used since the last batch; such an entry must still follow the weights when it is
    used again, two updates later."""
    from tg_hip import ops as O
    layer = Layer(dev, S3, 600)
    used, idle = [(S3_A, O.WPREP_FWD)], [(S3_B, O.WPREP_FWD), (S3_A, O.WPREP_DGRAD)]
    layer.require_prepared(used + idle)
    r_idle0 = layer.check(idle, "first use (idle entries)")
    layer.check(used, "first use")
    for i in range(3):
        layer.w.data.add_(0.0625 * (i + 1))
        O.weights_updated([layer.w])
        if batch:
            assert layer.entry(*used[0])[3], "the used entry is expected to be batchable"
            if i >= 1:
                for bhw, mode in idle:
                    assert layer.entry(bhw, mode)[4] is False          # not used since the first batch: the later ones skip it
        layer.check(used, f"update {i}")
    moved(r_idle0, layer.check(idle, "idle entries after three updates"))


def test_precision_round_trip(dev, batch):
    """f32, bf16, f32 on one weight: the precision is part of the key, so neither entry may serve the other."""
    from tg_hip import ops as O
    assert O.get_precision() == "f32"
    layer = Layer(dev, S3, 700)
    uses = uses_s3()
    try:
        layer.require_prepared(uses)
        layer.check(uses, "f32")
        y32 = [layer.run(bhw, mode).clone() for bhw, mode in uses]
        e32 = [layer.entry(bhw, mode) for bhw, mode in uses]
        O.set_precision("bf16")
        layer.require_prepared(uses)
        yb = [layer.run(bhw, mode).clone() for bhw, mode in uses]
        yb_hit = [layer.run(bhw, mode).clone() for bhw, mode in uses]
        O.WPREP_CACHE = False
        try:
            yb0 = [layer.run(bhw, mode).clone() for bhw, mode in uses]
        finally:
            O.WPREP_CACHE = True
        for (bhw, mode), a, a2, b, f in zip(uses, yb, yb_hit, yb0, y32):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"bf16 through the cache differs from the cache-off call {bhw, mode}"
            assert torch.equal(a2.view(torch.int32), b.view(torch.int32)), f"bf16 cache hit differs from the cache-off call {bhw, mode}"
            assert layer.entry(bhw, mode) is not None and layer.entry(bhw, mode)[2] is not None
            if mode == O.WPREP_FWD:          # (Winograd with bf16 operands; the Cin = 32 dgrad runs the fp32 gather launch under
                                             # either precision and gives the same bits: only its key differs)
                assert not torch.equal(a, f), f"bf16 and f32 results are expected to differ (else the switch is not exercised) {bhw, mode}"
        O.set_precision("f32")
        for (bhw, mode), f in zip(uses, y32):
            assert torch.equal(layer.run(bhw, mode).view(torch.int32), f.view(torch.int32)), "f32 after the bf16 excursion differs"
        layer.check(uses, "f32 again")
        # and an update made while the other precision was in use reaches both
        O.set_precision("bf16")
        layer.w.data.mul_(1.5)
        O.weights_updated([layer.w])
        yb1 = [layer.run(bhw, mode).clone() for bhw, mode in uses]
        O.WPREP_CACHE = False
        try:
            yb2 = [layer.run(bhw, mode).clone() for bhw, mode in uses]
        finally:
            O.WPREP_CACHE = True
        for a, b in zip(yb1, yb2):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "bf16 after an update differs from the cache-off call"
        O.set_precision("f32")
        layer.check(uses, "f32 after an update made under bf16")
    finally:
        O.set_precision("f32")
        O.WPREP_CACHE = True


def test_recycled_weight_address(dev, batch):
    """A weight is freed and the allocator hands its block to another weight of the same shape: same pointer, same _version,
    same out-of-band stamp -- only the entry's weak reference tells the two apart."""
    from tg_hip import ops as O
    layer = Layer(dev, S3, 800)
    uses = uses_s3()
    layer.require_prepared(uses)
    keep, reused = [], False
    for _try in range(8):
        r0 = layer.check(uses, "first weight")
        ptr, ver = layer.w.data_ptr(), layer.w._version
        layer.w = None
        w2 = layer.new_weight()
        layer.w = w2
        if w2.data_ptr() == ptr:
            assert w2._version == ver
            reused = True
            break
        keep.append(w2)
    assert reused, "the allocator never handed the freed weight's block out again in 8 tries"
    assert all(layer.entry(bhw, mode) is not None for bhw, mode in uses), "the old entries are expected to sit under the same keys"
    moved(r0, layer.check(uses, "second weight at the first one's address"))
