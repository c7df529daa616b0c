"""CPU check of the workspace contract of tg_conv_wgrad (include/terragan_hip.h: `ws` of tg_conv_wgrad_ws_bytes bytes is enough).

The small-channel weight-gradient routes of terra-gan_amd/csrc/smallconv.hip write one partial slab per workgroup; how many
workgroups they launch depends on the whole geometry (B, Ho, Wo, stride, pad), not only on the channel counts.  This test
recomputes, from the block-count rules of those kernels, the extent a call writes into its workspace and asserts that the
host-side query covers it -- for the generator's enc1 and `final`, and the discriminator's first and last convolutions, over
B = 1..16 and odd and even sizes up to 1040.  No GPU: the query is host code.
"""
import ctypes as C

import pytest

from tg_hip import lib as L

# smallconv.hip:21 (C1_T) and :327 (T1_TH, T1_TW): output tile edges of the Cin == 1 and the 64 -> 1 LDS kernels
C1_T, T1_TH, T1_TW = 16, 4, 16


def cdiv(a, b):
    return -(-a // b)


def align_up(n, a):
    return cdiv(n, a) * a


def colsum_ws_floats(rows, c):
    """tg_colsum_ws_floats (pointwise.hip:215): one partial row per workgroup of col_geom (pointwise.hip:35)."""
    cpp = min(c, 256)
    rlanes = 256 // cpp
    want = min(max(cdiv(rows, rlanes * 16), 1), 1024)
    rows_per_block = cdiv(rows, want)
    return align_up(cdiv(rows, rows_per_block) * c, 64)


def smallconv_wgrad_extent(B, H, W, cin, ho, wo, cout, k, stride, pad):
    """Floats of workspace the small-channel wgrad route writes for this geometry (db requested), or None when the geometry
    does not take that route (smallconv_wgrad_applies, smallconv.hip:1119)."""
    mpix = B * ho * wo
    if cin == 1 and cout % 64 == 0 and k in (3, 4, 7):
        # c1_wgrad_blocks (smallconv.hip:1109): one workgroup per 16 x 16 output tile, at most 512; the weight partials
        # [nb][Cout][k][k] are followed by the bias partials [nb][Cout] (smallconv.hip:1166), which replace the column sum
        nb = min(cdiv(wo, C1_T) * cdiv(ho, C1_T) * B, 512)
        return nb * cout * k * k + nb * cout
    if cout == 1 and cin % 256 == 0 and cin <= 1024 and k in (3, 4) and stride == 1:
        # to1w_wgrad_ok (smallconv.hip:1098): one workgroup per (image, band of 4 output rows)
        nb = B * cdiv(ho, 4)
    elif cout == 1 and cin == 64 and wo % 4 == 0 and k in (3, 4):
        if k == 3 and stride == 1 and pad == 1 and ho >= T1_TH and wo >= T1_TW:
            # to1_wgrad_lds_ok (smallconv.hip:1114): one workgroup per 4 x 16 output tile, at most 768
            nb = min(cdiv(wo, T1_TW) * cdiv(ho, T1_TH) * B, 768)
        else:
            # to1_wgrad_blocks (smallconv.hip:1103): quads of output pixels dealt to at most 1024 workgroups
            quads = mpix // 4
            qpb = cdiv(quads, min(max(cdiv(quads, 64), 1), 1024))
            nb = cdiv(quads, qpb) if qpb else 1
    else:
        return None
    # the bias gradient is a column sum behind the slabs (conv_wgrad_impl, igemm.hip: align_up(smallconv_wgrad_ws_floats, 64))
    off = align_up(nb * cout * k * k * cin + 64, 64)
    return off + colsum_ws_floats(mpix, cout)


# (name, Cin, Cout, k, stride, pad): generator.py / discriminator.py, engine.py G_ENC / D_LAYERS
LAYERS = [("enc1", 1, 64, 7, 2, 3), ("d_conv0", 1, 64, 4, 2, 1), ("final", 64, 1, 3, 1, 1), ("d_last", 512, 1, 4, 1, 1)]
SIZES = sorted(set(range(5, 1041, 53)) | set(range(8, 1041, 56)) | {16, 17, 40, 72, 448, 488, 640, 976, 1040})


def _sweep(name, cin, cout, k, stride, pad):
    lib = L.load()
    bad = []
    n = 0
    for B in range(1, 17):
        for h in SIZES:
            for w in {h, 2 * h, max(h // 2, 1)}:
                if w > 1040 * 2:
                    continue
                ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
                if ho < 1 or wo < 1:
                    continue
                ext = smallconv_wgrad_extent(B, h, w, cin, ho, wo, cout, k, stride, pad)
                if ext is None:
                    continue
                n += 1
                g = L.TgConv(B, h, w, cin, ho, wo, cout, k, stride, pad, 0)
                got = lib.tg_conv_wgrad_ws_bytes(C.byref(g))
                if got < 4 * ext:
                    bad.append((B, h, w, got // 4, ext))
    return n, bad


@pytest.mark.parametrize("layer", LAYERS, ids=[x[0] for x in LAYERS])
def test_wgrad_ws_query_covers_smallconv_extent(layer):
    n, bad = _sweep(*layer)
    assert n > 500, n
    assert not bad, f"{layer[0]}: {len(bad)} of {n} geometries under-reported, e.g. (B, H, W, reported, written floats) {bad[:5]}"


def test_wgrad_ws_query_issue_examples():
    """The geometries the under-sizing was first found at: enc1 / D conv0 at 488 x 976 and 448^2, `final` on small tiles."""
    lib = L.load()
    cases = [(1, 488, 976) + LAYERS[0][1:], (3, 448, 448) + LAYERS[0][1:], (3, 448, 448) + LAYERS[1][1:],
             (1, 16, 16) + LAYERS[2][1:], (3, 72, 40) + LAYERS[2][1:], (16, 256, 256) + LAYERS[2][1:]]
    for B, h, w, cin, cout, k, s, p in cases:
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        ext = smallconv_wgrad_extent(B, h, w, cin, ho, wo, cout, k, s, p)
        got = lib.tg_conv_wgrad_ws_bytes(C.byref(L.TgConv(B, h, w, cin, ho, wo, cout, k, s, p, 0)))
        assert got >= 4 * ext, ((B, h, w, cin, cout, k), got // 4, ext)


def test_split_k_room_is_promised():
    """fwd / dgrad queries promise 64 output slabs (capped at 64 Mi floats) of split-K room beyond their weight scratch: the
    planners use no more than that, so a caller handing the queried size gets the same split counts as a larger buffer."""
    lib = L.load()
    for B, h, cin, cout, k, s, p in [(16, 4, 512, 512, 3, 2, 1), (16, 2, 1024, 512, 3, 1, 1), (1, 16, 256, 512, 3, 1, 1)]:
        ho = (h + 2 * p - k) // s + 1
        g = L.TgConv(B, h, h, cin, ho, ho, cout, k, s, p, 0)
        assert lib.tg_conv_fwd_ws_bytes(C.byref(g)) >= 4 * 64 * B * ho * ho * cout
        assert lib.tg_conv_dgrad_ws_bytes(C.byref(g)) >= 4 * 64 * B * h * h * cin
