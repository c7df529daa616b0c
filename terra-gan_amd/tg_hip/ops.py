"""Tensor-level wrappers over the C ABI.  Tensors are fp32 HIP tensors, activations laid out
[B][H][W][C] (contiguous), conv weights logical OIHW stored channels_last (= [Cout][kh][kw][Cin]).
Torch is used for allocation and the stream handle only; every arithmetic op is a HIP kernel."""
import ctypes as C

import numpy as np
import torch

from . import lib as L

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
PREC_F32, PREC_BF16, PREC_F32_WINO4 = 0, 1, 2
_precision = PREC_F32


def set_precision(name):
    """'f32' (default) or 'bf16': arithmetic of the conv inner products (bf16 operands, fp32 accumulate; everything in
    memory stays fp32).  Process-wide switch used by bench.py / train(config) for BASELINE config 3."""
    global _precision
    _precision = {"f32": PREC_F32, "fp32": PREC_F32, "bf16": PREC_BF16}[name]


def get_precision():
    return "bf16" if _precision == PREC_BF16 else "f32"
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
PROF_TAGS = False        # bench.py's instrumented pass: label conv launches with their layer (tg_prof_tag)


def tag(name):
    if PROF_TAGS:
        _lib().tg_prof_tag(name.encode())

_ws = {}


def _lib():
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t, name="tensor"):
    if t is None:
        return
    if not t.is_cuda:
        raise L.TgError(f"{name}: expected a HIP (cuda) tensor -- there is no CPU path")
    if t.dtype != torch.float32:
        raise L.TgError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise L.TgError(f"{name}: expected a contiguous tensor, strides {t.stride()}")


def _same_numel(ref, ref_name, **others):
    """Every given tensor (None is skipped) holds as many elements as `ref`: the kernels index them all by ref's count."""
    for name, t in others.items():
        if t is not None and t.numel() != ref.numel():
            raise L.TgError(f"{name}: {t.numel()} elements {tuple(t.shape)}, but {ref_name} has {ref.numel()} {tuple(ref.shape)}")


def _chk_scalar(t, name):
    _chk(t, name)
    if t is not None and t.numel() != 1:
        raise L.TgError(f"{name}: expected one float, got {t.numel()} elements")


def workspace(nbytes):
    """Stream-ordered scratch shared by all ops on (device, stream); grown on demand."""
    dev = torch.cuda.current_device()
    key = (dev, torch.cuda.current_stream().cuda_stream)
    buf = _ws.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        n = max(int(nbytes) // 4 + 64, 1 << 20)
        buf = torch.empty(n, dtype=torch.float32, device=f"cuda:{dev}")
        _ws[key] = buf
    return buf


def empty(*shape, like=None, device=None):
    return torch.empty(*shape, dtype=torch.float32, device=like.device if like is not None else device)


def weight_view(w):
    """[Cout][kh][kw][Cin] view of an OIHW parameter stored channels_last; converts the storage
    in place (once) if the parameter is not laid out that way yet."""
    v = w.detach().permute(0, 2, 3, 1)
    if not v.is_contiguous():
        w.data = w.data.contiguous(memory_format=torch.channels_last)
        v = w.detach().permute(0, 2, 3, 1)
        if not v.is_contiguous():          # ambiguous strides (Cin == 1 or k == 1): force a dense OHWI buffer
            dense = v.contiguous()
            w.data = dense.permute(0, 3, 1, 2)
            v = w.detach().permute(0, 2, 3, 1)
    return v


def _prec(wino4):
    """TG_PREC_F32_WINO4 (Winograd F(4x4,3x3) where the geometry allows: the frozen VGG trunk) only refines fp32 mode."""
    return PREC_F32_WINO4 if (wino4 and _precision == PREC_F32) else _precision


def conv_geom(x, cout, k, stride, pad, wino4=False):
    B, H, W, Cin = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return L.TgConv(B, H, W, Cin, Ho, Wo, cout, k, stride, pad, _prec(wino4))


# ---- prepared weights (tg_conv_wprep): computed when a weight tensor is first used and again only after it changed --------
WPREP_FWD, WPREP_DGRAD = 0, 1
WPREP_CACHE = True            # False: every conv call prepares its weights in the workspace (the round-1 behaviour)
WPREP_VERIFY = __import__("os").environ.get("TG_WPREP_VERIFY") == "1"      # debug: re-prepare and compare on every cache hit
WPREP_BATCH = True            # re-prepare all batchable entries of the updated weights in ONE launch right after the optimiser step
_wprep = {}                   # (weight ptr, mode, geometry) -> [weakref(weight), version stamp, prepared buffer or None,
                              #                                   batch descriptor (bytes) or False, used since the last batch]
_wstamp = {}                  # weight ptr -> number of out-of-band updates (kernels writing through raw pointers)
_wprep_tables = {}            # (device, concatenated descriptor bytes) -> device array of those descriptors
WPREP_TABLES_MAX = 16         # ... of which the most recently used stay
wprep_capture = None          # tg_hip.graph, while a step is captured: the WprepCapture of that graph


class WprepCapture:
    """What a captured step does with the prepared-weight cache.  `keys`: the entries whose batched preparation the graph
    replays (after its Adam).  `hits`: the batchable entries its convolutions read WITHOUT preparing them first -- the graph
    takes those buffers as the previous replay left them.  `refs`: the device tables the captured launches read."""

    def __init__(self):
        self.keys, self.hits, self.refs = [], [], []


def weights_updated(params):
    """REQUIRED after any parameter write torch's version counter does not see -- kernels writing through raw pointers
    (hip_adam_step does it itself), `.data` writes, custom broadcasts, user-side EMA / clamping through `.data`: the
    prepared-weight cache keeps its own stamp per storage and would otherwise keep convolving with stale transforms.
    TG_WPREP_VERIFY=1 (debug) re-prepares on every use and raises when a cached buffer was stale.
    A GraphedTrainStep honours the same protocol: before each replay it compares the stamps of the prepared buffers its
    graph reads with their weights' and re-prepares the stale ones (prepared_stale / prepare_keys)."""
    ptrs = set()
    for p in params:
        if p.dim() == 4:
            ptr = p.data_ptr()
            _wstamp[ptr] = _wstamp.get(ptr, 0) + 1
            ptrs.add(ptr)
    if WPREP_BATCH and WPREP_CACHE and ptrs:
        _prepare_batch(ptrs)


def _prepare_batch(ptrs):
    """The prepared forms of the weights at `ptrs` that were used since the last batch, recomputed by ONE launch
    (tg_conv_wprep_run over a cached device table of descriptors) instead of one launch per layer and mode at first use."""
    ents = []
    for key, e in _wprep.items():
        if key[0] in ptrs and e[3] and e[4] and e[0]() is not None:
            ents.append((key, e))
    _run_batch(ents)


def prepared_stale(keys):
    """Those of `keys` whose live entry does not carry its weight's current stamp: the weight was written (in place through
    torch, or out of band + weights_updated) or the buffer was re-prepared for an earlier value since the entry was stamped.
    Host-side comparisons only."""
    stale = []
    for key in keys:
        e = _wprep.get(key)
        w = e[0]() if e is not None else None
        if w is not None and e[1] != (w._version, _wstamp.get(key[0], 0)):
            stale.append(key)
    return stale


def prepare_keys(keys):
    """Re-prepare the batchable entries `keys` into their existing buffers by one launch on the current stream, whether or
    not they were used since the last batch (tg_hip.graph: a replay's forward reads them without going through _prepared)."""
    _run_batch([(key, _wprep[key]) for key in keys])


def _run_batch(ents):
    if not ents:
        return
    # keyed by the descriptors themselves (they hold the w / out pointers, mode and geometry): an id()-based key could be
    # recycled by CPython for a replaced entry and hit a stale table whose `out` points at a freed prepared buffer
    raw = b"".join(e[3] for _, e in ents)
    tkey = (ents[0][1][2].device, raw)
    table = _wprep_tables.pop(tkey, None)
    if table is None:
        import numpy as np
        table = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(ents[0][1][2].device)
        # the least recently used ones go, one at a time: emptying the cache here dropped the table the generator's step had made
        # a moment ago, and the capture that followed the warm-up step cannot build one (a host-to-device copy)
        while len(_wprep_tables) >= WPREP_TABLES_MAX:
            del _wprep_tables[next(iter(_wprep_tables))]
    _wprep_tables[tkey] = table                   # (re-inserted on a hit: the dict's order is the order of last use)
    L.check(_lib().tg_conv_wprep_run(C.c_void_p(table.data_ptr()), len(ents), _stream()), "tg_conv_wprep_run")
    for key, e in ents:
        e[1] = (e[0]()._version, _wstamp.get(key[0], 0))
        e[4] = False
    if wprep_capture is not None:
        wprep_capture.keys.extend(key for key, _e in ents)
        wprep_capture.refs.append(table)          # (_wprep_tables may be cleared while the graph still reads this one)


def graph_replayed(weight_ptrs, refreshed_keys):
    """A captured train step was replayed: the weights at `weight_ptrs` changed on the device behind the host's back.  Every
    prepared form of them is stale from here on -- entries made eagerly for another geometry (validation / inference at
    another size), and the non-batchable ones the graph re-prepares in its FORWARD, i.e. from the weights of before its
    Adam -- except those in `refreshed_keys`, which the replayed tg_conv_wprep_run launch has just recomputed."""
    for ptr in weight_ptrs:
        _wstamp[ptr] = _wstamp.get(ptr, 0) + 1
    for key in refreshed_keys:
        e = _wprep.get(key)
        if e is not None:
            w = e[0]()
            if w is not None:
                e[1] = (w._version, _wstamp.get(key[0], 0))


def _prepared(w, wv, g, mode):
    """Prepared form of weight `w` for (g, mode), or None when that path reads the raw weights."""
    if not WPREP_CACHE:
        return None
    import weakref
    ptr = wv.data_ptr()
    key = (ptr, mode, g.H, g.W, g.Cin, g.Cout, g.k, g.stride, g.pad, g.precision)
    stamp = (w._version, _wstamp.get(ptr, 0))
    ent = _wprep.get(key)
    if ent is not None and ent[0]() is w and ent[1] == stamp:
        ent[4] = True
        if wprep_capture is not None and ent[3]:
            wprep_capture.hits.append(key)
        if WPREP_VERIFY and ent[2] is not None:
            # (a copy, not an empty buffer: a dgrad buffer has room for the larger of the transposed and the transformed weights
            # and the preparation writes one of them -- the rest is never written and must not take part in the comparison)
            fresh = ent[2].clone()
            L.check(_lib().tg_conv_wprep(C.byref(g), mode, _p(wv), _p(fresh), _stream()), "tg_conv_wprep")
            if not torch.equal(fresh.view(torch.int32), ent[2].view(torch.int32)):
                raise L.TgError("prepared weights are stale: a parameter was rewritten without tg_hip.ops.weights_updated()")
        return ent[2]
    lib = _lib()
    if ent is None or ent[0]() is not w:            # first use (or the address was recycled for another tensor)
        nb = lib.tg_conv_wprep_bytes(C.byref(g), mode)
        buf = torch.empty((nb + 3) // 4, dtype=torch.float32, device=wv.device) if nb else None
        if len(_wprep) > 512:
            for k_ in [k_ for k_, e in _wprep.items() if e[0]() is None]:
                del _wprep[k_]
        item = False
        if buf is not None:
            raw = C.create_string_buffer(lib.tg_conv_wprep_item_bytes())
            if lib.tg_conv_wprep_item(C.byref(g), mode, _p(wv), _p(buf), raw):
                item = raw.raw
        ent = [weakref.ref(w), None, buf, item, True]
        _wprep[key] = ent
    if ent[2] is not None:
        L.check(lib.tg_conv_wprep(C.byref(g), mode, _p(wv), _p(ent[2]), _stream()), "tg_conv_wprep")
    ent[1] = stamp
    ent[4] = True
    return ent[2]


_sparse_tickets = {}


class SparseMaps:
    """Prediction-half tile maps of the VGG trunk for one [pred; target] batch (tg_vgg_sparse_map): maps[i] belongs to the i-th
    conv of the plan.  Holds the device buffer the maps point into.  for_bwd: built with the consumer's mask, so the maps also
    cover every pixel whose input gradient is read (maps[i].pix) and may steer the trunk's backward."""

    def __init__(self, buf, maps, for_bwd=False):
        self.buf, self.maps, self.for_bwd = buf, maps, for_bwd


def vgg_sparse_map(x, nb, plan, mask=None):
    """x: the trunk's 1-channel input [2 nb][H][W] (or [2 nb][H][W][1]).  plan: 'C' (3x3 / stride-1 / pad-1 conv) and 'M'
    (2x2 / stride-2 max-pool) in the trunk's order.  Returns SparseMaps, or None where no map can be built (the trunk then
    runs dense: the same values).  One launch, no host synchronisation.  mask [nb][H][W]: pixels with mask != 1 are marked as
    well (conv_dgrad(sparse=...), maxpool2_bwd_code(sparse=...))."""
    _chk(x, "x"); _chk(mask, "mask")
    H, W = x.shape[1], x.shape[2]
    assert x.shape[0] == 2 * nb and x.numel() == 2 * nb * H * W, (tuple(x.shape), nb)
    assert mask is None or (mask.numel() == nb * H * W and mask.shape[0] == nb), (tuple(mask.shape), nb, H, W)
    lib = _lib()
    pb = plan.encode()
    nbytes = lib.tg_vgg_sparse_map_bytes(nb, H, W, pb)
    if nbytes == 0:
        return None
    dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
    ticket = _sparse_tickets.get(dev)
    if ticket is None or ticket.numel() < nb + 1:
        if torch.cuda.is_current_stream_capturing():
            return None                 # (the zeroed tickets must outlive any capture: allocated by an eager call first)
        ticket = _sparse_tickets[dev] = torch.zeros(max(nb + 1, 64), dtype=torch.int32, device=x.device)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    nconv = plan.count("C")
    maps = (L.TgSparseMap * nconv)()
    L.check(lib.tg_vgg_sparse_map(_p(x), _p(mask), nb, H, W, pb, _p(buf), nbytes, _p(ticket), maps, _stream()), "tg_vgg_sparse_map")
    return SparseMaps(buf, maps, for_bwd=mask is not None)


def conv_fwd(x, w, bias, k, stride, pad, in_mask=None, ratio=None, act=ACT_NONE, slope=0.0, wino4=False, pool=False, sparse=None):
    """pool=True: returns (y, maxpool2(y)) from one call (tg_conv_fwd_pool: the pooled tensor leaves the conv's output transform
    where the kernel allows, the pool kernel runs on y otherwise).  sparse: a TgSparseMap of this layer (vgg_sparse_map) -- x is
    a [pred; target] batch and only the prediction tiles it marks are computed (tg_conv_fwd_sparse); the same values."""
    _chk(x, "x"); _chk(bias, "bias"); _chk(in_mask, "in_mask"); _chk(ratio, "ratio")
    if sparse is not None:
        assert in_mask is None and ratio is None
        wv = weight_view(w)
        _chk(wv, "weight")
        g = conv_geom(x, wv.shape[0], k, stride, pad, wino4)
        y = empty(g.B, g.Ho, g.Wo, g.Cout, like=x)
        yp = empty(g.B, g.Ho // 2, g.Wo // 2, g.Cout, like=x) if pool else None
        lib = _lib()
        ws = workspace(lib.tg_conv_fwd_ws_bytes(C.byref(g)))
        L.check(lib.tg_conv_fwd_sparse(C.byref(g), _p(x), _p(wv), _p(_prepared(w, wv, g, WPREP_FWD)), _p(bias), act, slope, _p(y),
                                       _p(yp), None, C.byref(sparse), _p(ws), ws.numel() * 4, _stream()), "tg_conv_fwd_sparse")
        return (y, yp) if pool else y
    wv = weight_view(w)
    _chk(wv, "weight")
    g = conv_geom(x, wv.shape[0], k, stride, pad, wino4)
    assert wv.shape == (g.Cout, k, k, g.Cin), (tuple(wv.shape), g.Cout, k, g.Cin)
    y = empty(g.B, g.Ho, g.Wo, g.Cout, like=x)
    lib = _lib()
    nb = lib.tg_conv_fwd_ws_bytes(C.byref(g))
    ws = workspace(nb)
    if pool:
        yp = empty(g.B, g.Ho // 2, g.Wo // 2, g.Cout, like=x)
        L.check(lib.tg_conv_fwd_pool(C.byref(g), _p(x), _p(in_mask), _p(wv), _p(_prepared(w, wv, g, WPREP_FWD)), _p(bias), _p(ratio),
                                     act, slope, _p(y), _p(yp), _p(ws), ws.numel() * 4, _stream()), "tg_conv_fwd_pool")
        return y, yp
    L.check(lib.tg_conv_fwd_p(C.byref(g), _p(x), _p(in_mask), _p(wv), _p(_prepared(w, wv, g, WPREP_FWD)), _p(bias), _p(ratio),
                              act, slope, _p(y), _p(ws), ws.numel() * 4, _stream()), "tg_conv_fwd")
    return y


def _bn_act(in_bn):
    """(mean, rstd, gamma, beta[, act[, slope]]) -> TgBnAct (the tensors stay referenced by the caller's tuple)."""
    mean, rstd, gamma, beta = in_bn[:4]
    for t in (mean, rstd, gamma, beta):
        _chk(t, "in_bn")
    act = in_bn[4] if len(in_bn) > 4 else ACT_RELU
    slope = in_bn[5] if len(in_bn) > 5 else 0.0
    return L.TgBnAct(mean.data_ptr(), rstd.data_ptr(), gamma.detach().data_ptr(), beta.detach().data_ptr(), act, slope)


def conv_bnin_supported(x_shape, cout, k, stride, pad, wgrad=False):
    """Can conv_fwd_bnin / conv_wgrad_bnin take this layer (input = act(BN(x)) applied while the kernel stages x)?"""
    B, H, W, Cin = x_shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g = L.TgConv(B, H, W, Cin, Ho, Wo, cout, k, stride, pad, _precision)
    return bool(_lib().tg_conv_bnin_supported(C.byref(g), 1 if wgrad else 0))


def conv_fwd_bnin(x, in_bn, w, bias, k, stride, pad, act=ACT_NONE, slope=0.0):
    """conv(act_bn(BN(x)), w) + bias with the BatchNorm + activation of `in_bn` applied on load (tg_conv_fwd_bnin)."""
    _chk(x, "x"); _chk(bias, "bias")
    wv = weight_view(w)
    _chk(wv, "weight")
    g = conv_geom(x, wv.shape[0], k, stride, pad)
    y = empty(g.B, g.Ho, g.Wo, g.Cout, like=x)
    lib = _lib()
    ws = workspace(lib.tg_conv_fwd_ws_bytes(C.byref(g)))
    bn = _bn_act(in_bn)
    L.check(lib.tg_conv_fwd_bnin(C.byref(g), _p(x), C.byref(bn), _p(wv), _p(bias), act, slope, _p(y), _p(ws), ws.numel() * 4, _stream()),
            "tg_conv_fwd_bnin")
    return y


def conv_pool_code_supported(x_shape, cout):
    """Can conv_fwd_pool_code take this 3x3 / stride-1 / pad-1 layer (pooled tensor + code, conv output never written)?"""
    B, H, W, Cin = x_shape
    g = L.TgConv(B, H, W, Cin, H, W, cout, 3, 1, 1, _precision)
    return bool(_lib().tg_conv_pool_code_supported(C.byref(g)))


def conv_fwd_pool_code(x, w, bias, sparse=None):
    """3x3 / stride-1 / pad-1 conv -> ReLU -> 2x2 max-pool: returns (pooled, code); the full-resolution output is not written
    (tg_conv_fwd_pool_code).  code: uint8 [B][H/2][W/2][Cout], consumed by maxpool2_bwd_code.  sparse: as in conv_fwd."""
    _chk(x, "x"); _chk(bias, "bias")
    wv = weight_view(w)
    _chk(wv, "weight")
    g = conv_geom(x, wv.shape[0], 3, 1, 1)
    yp = empty(g.B, g.Ho // 2, g.Wo // 2, g.Cout, like=x)
    code = torch.empty((g.B, g.Ho // 2, g.Wo // 2, g.Cout), dtype=torch.uint8, device=x.device)
    lib = _lib()
    ws = workspace(lib.tg_conv_fwd_ws_bytes(C.byref(g)))
    if sparse is not None:
        L.check(lib.tg_conv_fwd_sparse(C.byref(g), _p(x), _p(wv), _p(_prepared(w, wv, g, WPREP_FWD)), _p(bias), ACT_RELU, 0.0, None,
                                       _p(yp), C.c_void_p(code.data_ptr()), C.byref(sparse), _p(ws), ws.numel() * 4, _stream()),
                "tg_conv_fwd_sparse")
        return yp, code
    L.check(lib.tg_conv_fwd_pool_code(C.byref(g), _p(x), _p(wv), _p(_prepared(w, wv, g, WPREP_FWD)), _p(bias), _p(yp),
                                      C.c_void_p(code.data_ptr()), _p(ws), ws.numel() * 4, _stream()), "tg_conv_fwd_pool_code")
    return yp, code


def maxpool2_bwd_code(dout, code, sparse=None, out=None):
    """Gradient in front of the fused conv's ReLU from the pooled gradient and the pool code: [B][2 Ho][2 Wo][C].
    sparse: the TgSparseMap of the pooled conv -- only the 16x16 tiles it lists are written, the rest of the result is
    uninitialised memory (tg_maxpool2_bwd_code_sparse)."""
    _chk(dout, "dout"); _chk(out, "out")
    B, Ho, Wo, Cc = dout.shape
    assert code.dtype == torch.uint8 and code.is_contiguous() and tuple(code.shape[1:]) == (Ho, Wo, Cc) and code.shape[0] >= B
    dx = out if out is not None else empty(B, 2 * Ho, 2 * Wo, Cc, like=dout)
    assert tuple(dx.shape) == (B, 2 * Ho, 2 * Wo, Cc)
    if sparse is not None:
        L.check(_lib().tg_maxpool2_bwd_code_sparse(_p(dout), C.c_void_p(code.data_ptr()), B, Ho, Wo, Cc, _p(dx), C.byref(sparse), _stream()),
                "tg_maxpool2_bwd_code_sparse")
        return dx
    L.check(_lib().tg_maxpool2_bwd_code(_p(dout), C.c_void_p(code.data_ptr()), B, Ho, Wo, Cc, _p(dx), _stream()), "tg_maxpool2_bwd_code")
    return dx


def conv_dgrad_sparse_planned(x_shape, cout, sparse, gate=0):
    """Will conv_dgrad(sparse=...) of a 3x3 / stride-1 / pad-1 layer write only the listed tiles (True) or fall back to the dense
    launch (False)?  gate: 0 none, 1 `gate`, 2 `gate_bits`.  The launch's own plan; no GPU work."""
    B, H, W, Cin = x_shape
    g = L.TgConv(B, H, W, Cin, H, W, cout, 3, 1, 1, _precision)
    return bool(_lib().tg_conv_dgrad_sparse_planned(C.byref(g), gate, C.byref(sparse)))


def relu_gate_pack(a, nb=None):
    """ReLU gates of the first `nb` images of an NHWC activation [B][H][W][C] (C % 32 == 0) in one bit per element:
    uint32 [nb][H][W][C/32], bit c % 32 of word c / 32 = (a > 0) -- the predicate of conv_dgrad's fp32 gate (tg_relu_gate_pack)."""
    _chk(a, "a")
    B, H, W, Cc = a.shape
    nb = B if nb is None else nb
    assert 0 < nb <= B, (nb, B)
    bits = torch.empty((nb, H, W, Cc // 32), dtype=torch.uint32, device=a.device)
    L.check(_lib().tg_relu_gate_pack(_p(a), nb * H * W, Cc, C.c_void_p(bits.data_ptr()), _stream()), "tg_relu_gate_pack")
    return bits


def conv_dgrad(dy, w, x_shape, k, stride, pad, in_mask=None, out=None, gate=None, gate_act=ACT_RELU, gate_slope=0.0, wino4=False,
               gate_bits=None, sparse=None):
    """dx for an input of shape x_shape=[B,H,W,Cin]; accumulates into `out` when given.  `gate` = output of the
    activation that produced x: its backward is fused into the epilogue (dx *= act'(gate)).  `gate_bits` = relu_gate_pack of a
    ReLU output in place of `gate` (exclusive with it): the same dx bit for bit (tg_conv_dgrad_gbits).
    sparse: the TgSparseMap of this conv's OUTPUT (vgg_sparse_map with a mask): only the tiles it lists are written where the
    launch can do so -- the rest of dx is then uninitialised memory -- and `out` is overwritten, not accumulated into; with
    Cin == 1 every pixel is written, 0.0 outside the map's needed pixels (tg_conv_dgrad_sparse)."""
    _chk(dy, "dy"); _chk(in_mask, "in_mask"); _chk(out, "out"); _chk(gate, "gate")
    wv = weight_view(w)
    B, H, W, Cin = x_shape
    g = L.TgConv(B, H, W, Cin, dy.shape[1], dy.shape[2], dy.shape[3], k, stride, pad, _prec(wino4))
    acc = 1 if out is not None else 0
    dx = out if out is not None else empty(B, H, W, Cin, like=dy)
    lib = _lib()
    ws = workspace(lib.tg_conv_dgrad_ws_bytes(C.byref(g)))
    if sparse is not None:
        assert in_mask is None and not wino4 and tuple(dx.shape) == tuple(x_shape)
        assert gate is None or (gate_bits is None and tuple(gate.shape) == tuple(x_shape))
        if gate_bits is not None:
            assert gate_bits.dtype == torch.uint32 and gate_bits.is_contiguous() and tuple(gate_bits.shape) == (B, H, W, Cin // 32), \
                (gate_bits.dtype, tuple(gate_bits.shape), tuple(x_shape))
        L.check(lib.tg_conv_dgrad_sparse(C.byref(g), _p(dy), _p(wv), _p(_prepared(w, wv, g, WPREP_DGRAD)), _p(gate),
                                         gate_act if gate is not None else ACT_NONE, gate_slope,
                                         C.c_void_p(gate_bits.data_ptr()) if gate_bits is not None else None, _p(dx),
                                         C.byref(sparse), _p(ws), ws.numel() * 4, _stream()), "tg_conv_dgrad_sparse")
        return dx
    if gate_bits is not None:
        assert gate is None and out is None, "conv_dgrad: gate_bits is exclusive with gate and does not accumulate"
        assert gate_bits.dtype == torch.uint32 and gate_bits.is_contiguous() and tuple(gate_bits.shape) == (B, H, W, Cin // 32), \
            (gate_bits.dtype, tuple(gate_bits.shape), tuple(x_shape))
        L.check(lib.tg_conv_dgrad_gbits(C.byref(g), _p(dy), _p(wv), _p(_prepared(w, wv, g, WPREP_DGRAD)), _p(in_mask),
                                        C.c_void_p(gate_bits.data_ptr()), _p(dx), 0, _p(ws), ws.numel() * 4, _stream()),
                "tg_conv_dgrad_gbits")
        return dx
    if gate is not None:
        assert out is None and tuple(gate.shape) == tuple(x_shape)
    L.check(lib.tg_conv_dgrad_p(C.byref(g), _p(dy), _p(wv), _p(_prepared(w, wv, g, WPREP_DGRAD)), _p(in_mask), _p(gate),
                                gate_act if gate is not None else ACT_NONE, gate_slope, _p(dx), acc, _p(ws), ws.numel() * 4,
                                _stream()), "tg_conv_dgrad")
    return dx


def conv_wgrad(x, dy, w, k, stride, pad, in_mask=None, want_bias=True, dw_out=None, db_out=None, in_bn=None):
    """Returns (dw, db): dw has the parameter's logical shape AND strides (channels_last).  dw_out / db_out:
    preallocated destinations (persistent gradient buffers) with the parameter's layout.
    in_bn: the layer's input is act(BN(x)), applied on load (tg_conv_wgrad_bnin; see conv_bnin_supported)."""
    _chk(x, "x"); _chk(dy, "dy"); _chk(in_mask, "in_mask")
    wv = weight_view(w)
    B, H, W, Cin = x.shape
    g = L.TgConv(B, H, W, Cin, dy.shape[1], dy.shape[2], dy.shape[3], k, stride, pad, _precision)
    if dw_out is not None:
        dwv = dw_out.permute(0, 2, 3, 1)
        assert dwv.is_contiguous() and dwv.shape == wv.shape
    else:
        dwv = torch.empty_like(wv)                   # [Cout][k][k][Cin] contiguous
    db = (db_out if db_out is not None else empty(g.Cout, like=x)) if want_bias else None
    lib = _lib()
    ws = workspace(lib.tg_conv_wgrad_ws_bytes(C.byref(g)))
    if in_bn is not None:
        assert in_mask is None
        bn = _bn_act(in_bn)
        L.check(lib.tg_conv_wgrad_bnin(C.byref(g), _p(x), C.byref(bn), _p(dy), _p(dwv), _p(db), _p(ws), ws.numel() * 4, _stream()),
                "tg_conv_wgrad_bnin")
        return dwv.permute(0, 3, 1, 2), db
    L.check(lib.tg_conv_wgrad(C.byref(g), _p(x), _p(in_mask), _p(dy), _p(dwv), _p(db), _p(ws), ws.numel() * 4, _stream()),
            "tg_conv_wgrad")
    return dwv.permute(0, 3, 1, 2), db


def fold_cin(w):
    """[Cout,Cin,k,k] -> [Cout,1,k,k] channel-summed kernel (grey image repeated xCin)."""
    wv = weight_view(w)
    co, kh, kw, ci = wv.shape
    out = empty(co, kh, kw, 1, like=wv)
    L.check(_lib().tg_fold_cin(_p(wv), co, kh * kw, ci, _p(out), _stream()), "tg_fold_cin")
    return out.permute(0, 3, 1, 2)


def mask_update(mask, k, stride, pad):
    _chk(mask, "mask")
    B, H, W = mask.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    mo, ratio = empty(B, Ho, Wo, like=mask), empty(B, Ho, Wo, like=mask)
    L.check(_lib().tg_mask_update(_p(mask), B, H, W, k, stride, pad, Ho, Wo, _p(mo), _p(ratio), _stream()), "tg_mask_update")
    return mo, ratio


def mask_up_merge(up_mask, skip_mask):
    _chk(up_mask, "up_mask"); _chk(skip_mask, "skip_mask")
    B, h, w = up_mask.shape
    _, H, W = skip_mask.shape
    out = torch.empty_like(skip_mask)
    L.check(_lib().tg_mask_up_merge(_p(up_mask), _p(skip_mask), B, h, w, H, W, _p(out), _stream()), "tg_mask_up_merge")
    return out


MASK_FUSE_PIXELS = 64 * 64


def mask_pyramid(mask, enc, dec):
    """Every mask of one generator forward from ONE launch (tg_mask_pyramid).  enc / dec: [(k, stride, pad), ...] of the
    encoder / decoder partial convs (generator.py:13-28).  Returns (m, er, dmasks, dr) exactly as the per-level calls
    would: m[i] / er[i] = mask / ratio after encoder layer i (m[0] = input, er[0] = None), dmasks[j] = merged mask fed to
    decoder layer j (generator.py:51-54,68-74), dr[j] = its ratio map.  Bit-identical to mask_update / mask_up_merge."""
    _chk(mask, "mask")
    B, H, W = mask.shape
    ne, nd = len(enc), len(dec)
    dims = [(H, W)]
    for (k, s, p) in enc:
        h, w = dims[-1]
        dims.append(((h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1))
    # decoder level j merges the current decoder mask (upsampled x2) with skip mask m[ne-1-j] (the input mask for the last)
    sizes = [B * h * w for (h, w) in dims[1:]] * 2
    ddims = []
    cur = dims[ne]
    for j, (k, s, p) in enumerate(dec):
        sk = dims[ne - 1 - j]
        ddims.append((cur, sk))
        cur = ((sk[0] + 2 * p - k) // s + 1, (sk[1] + 2 * p - k) // s + 1)
        sizes += [B * sk[0] * sk[1], B * cur[0] * cur[1], B * cur[0] * cur[1]]
    # one allocation, every map starting on a 256-byte boundary
    offs, tot = [], 0
    for n in sizes:
        offs.append(tot)
        tot += (n + 63) // 64 * 64
    buf = torch.empty(tot, dtype=torch.float32, device=mask.device)
    it = iter(zip(offs, sizes))

    def view(shape):
        o, n = next(it)
        return buf[o:o + n].view(shape)

    m, er = [mask], [None]
    mo_views = [view((B,) + dims[i + 1]) for i in range(ne)]
    r_views = [view((B,) + dims[i + 1]) for i in range(ne)]
    # A level with few pixels per image is pure launch latency: runs of such levels go into ONE launch in which a single
    # workgroup per image walks them (tg_mask_pyramid); a large level (> MASK_FUSE_PIXELS outputs per image) needs the whole
    # chip and keeps its own launch.  At 256x256: enc1 | enc2 ... enc7, dec7 ... dec3 (16 ops) | dec2 x 2 | dec1 x 2.
    pm = L.TgMaskPyramid()
    n_ops = 0
    lib = _lib()

    def flush():
        nonlocal n_ops, pm
        if n_ops:
            pm.nops = n_ops
            L.check(lib.tg_mask_pyramid(C.byref(pm), B, _stream()), "tg_mask_pyramid")
            pm, n_ops = L.TgMaskPyramid(), 0

    def put(kind, hin, hout, k, s, p, a, a2, o, o2):
        nonlocal n_ops
        if hout[0] * hout[1] > MASK_FUSE_PIXELS:
            flush()
            if kind == 0:
                L.check(lib.tg_mask_update(_p(a), B, hin[0], hin[1], k, s, p, hout[0], hout[1], _p(o), _p(o2), _stream()), "tg_mask_update")
            else:
                L.check(lib.tg_mask_up_merge(_p(a), _p(a2), B, hin[0], hin[1], hout[0], hout[1], _p(o), _stream()), "tg_mask_up_merge")
            return
        if n_ops == L.TG_MASK_PYRAMID_MAX:
            flush()
        op = pm.op[n_ops]
        op.kind, op.H, op.W, op.Ho, op.Wo, op.k, op.stride, op.pad = kind, hin[0], hin[1], hout[0], hout[1], k, s, p
        op.in_, op.in2, op.out, op.out2 = a.data_ptr(), (a2.data_ptr() if a2 is not None else None), o.data_ptr(), \
            (o2.data_ptr() if o2 is not None else None)
        n_ops += 1

    for i, (k, s, p) in enumerate(enc):
        put(0, dims[i], dims[i + 1], k, s, p, m[-1], None, mo_views[i], r_views[i])
        m.append(mo_views[i])
        er.append(r_views[i])
    dm, dmasks, dr = m[ne], [], []
    for j, (k, s, p) in enumerate(dec):
        (hin, sk) = ddims[j]
        skip_m = m[ne - 1 - j]
        mm = view((B,) + sk)
        hout = ((sk[0] + 2 * p - k) // s + 1, (sk[1] + 2 * p - k) // s + 1)
        mo, r = view((B,) + hout), view((B,) + hout)
        put(1, hin, sk, 0, 0, 0, dm, skip_m, mm, None)
        put(0, sk, hout, k, s, p, mm, None, mo, r)
        dmasks.append(mm)
        dr.append(r)
        dm = mo
    flush()
    return m, er, dmasks, dr


BN_SMALL_ROWS = 2048          # tg_bn_fwd / tg_bn_act_bwd take their one-launch form up to this many rows (pointwise.hip)


def bn_stats(y, running_mean=None, running_var=None, nbt=None, eps=BN_EPS, momentum=BN_MOMENTUM):
    _chk(y, "y")
    Cc = y.shape[-1]
    rows = y.numel() // Cc
    mean, rstd = empty(Cc, like=y), empty(Cc, like=y)
    lib = _lib()
    ws = workspace(lib.tg_bn_ws_bytes(rows, Cc))
    nbt_p = None if nbt is None else C.c_void_p(nbt.data_ptr())
    L.check(lib.tg_bn_stats(_p(y), rows, Cc, eps, momentum, _p(mean), _p(rstd), _p(running_mean), _p(running_var), nbt_p,
                            _p(ws), ws.numel() * 4, _stream()), "tg_bn_stats")
    return mean, rstd


def bn_fwd(y, gamma, beta, act, slope=0.0, running_mean=None, running_var=None, nbt=None, out=None, eps=BN_EPS,
           momentum=BN_MOMENTUM, apply=True):
    """Training-mode BatchNorm forward: (mean, rstd, out) = bn_stats + bn_act_fwd in one call (one launch on small maps).
    apply=False: statistics (and running-statistics update) only, out = None -- the consumer applies the affine map + activation
    while it loads y (conv_fwd_bnin / conv_wgrad_bnin)."""
    _chk(y, "y"); _chk(out, "out")
    Cc = y.shape[-1]
    rows = y.numel() // Cc
    mean, rstd = empty(Cc, like=y), empty(Cc, like=y)
    if out is None and apply:
        out = torch.empty_like(y)
    lib = _lib()
    ws = workspace(lib.tg_bn_ws_bytes(rows, Cc))
    nbt_p = None if nbt is None else C.c_void_p(nbt.data_ptr())
    L.check(lib.tg_bn_fwd(_p(y), rows, Cc, eps, momentum, _p(gamma.detach()), _p(beta.detach()), act, slope, _p(mean), _p(rstd),
                          _p(running_mean), _p(running_var), nbt_p, _p(out), _p(ws), ws.numel() * 4, _stream()), "tg_bn_fwd")
    return mean, rstd, out


def bn_eval_stats(running_mean, running_var, eps=BN_EPS):
    Cc = running_mean.numel()
    mean, rstd = torch.empty_like(running_mean), torch.empty_like(running_mean)
    L.check(_lib().tg_bn_eval_stats(_p(running_mean), _p(running_var), Cc, eps, _p(mean), _p(rstd), _stream()), "tg_bn_eval_stats")
    return mean, rstd


def bn_running_update(mean, rstd, rows, running_mean, running_var, nbt, eps=BN_EPS, momentum=BN_MOMENTUM):
    nbt_p = None if nbt is None else C.c_void_p(nbt.data_ptr())
    L.check(_lib().tg_bn_running_update(_p(mean), _p(rstd), rows, mean.numel(), eps, momentum, _p(running_mean),
                                        _p(running_var), nbt_p, _stream()), "tg_bn_running_update")


def bn_fwd_grouped(y, groups, gamma, beta, act, slope=0.0, out=None, eps=BN_EPS):
    """Training-mode BatchNorm of `groups` passes stacked along the leading dimension, statistics per pass, in one set of launches
    (tg_bn_fwd_grouped).  -> (mean [groups, C], rstd [groups, C], out).  No running-statistics update (bn_running_update_multi)."""
    _chk(y, "y"); _chk(out, "out")
    Cc = y.shape[-1]
    rows_g = y.numel() // Cc // groups
    assert rows_g * groups * Cc == y.numel() and y.shape[0] % groups == 0
    mean, rstd = empty(groups, Cc, like=y), empty(groups, Cc, like=y)
    if out is None:
        out = torch.empty_like(y)
    lib = _lib()
    ws = workspace(lib.tg_bn_grouped_ws_bytes(rows_g, groups, Cc))
    L.check(lib.tg_bn_fwd_grouped(_p(y), rows_g, groups, Cc, eps, _p(gamma.detach()), _p(beta.detach()), act, slope, _p(mean), _p(rstd),
                                  _p(out), _p(ws), ws.numel() * 4, _stream()), "tg_bn_fwd_grouped")
    return mean, rstd, out


def bn_act_bwd_grouped(dout, y, groups, mean, rstd, gamma, beta, act, slope=0.0, want_dbias=True, outs=None):
    """Backward of bn_fwd_grouped, in place on dout.  -> (dy, dgamma, dbeta, dbias): parameter gradients summed over the passes."""
    _chk(dout, "dout"); _chk(y, "y"); _chk(mean, "mean"); _chk(rstd, "rstd")
    Cc = y.shape[-1]
    rows_g = y.numel() // Cc // groups
    if outs is not None:
        dgamma, dbeta, dbias = outs
    else:
        dgamma, dbeta = empty(Cc, like=y), empty(Cc, like=y)
        dbias = empty(Cc, like=y) if want_dbias else None
    lib = _lib()
    ws = workspace(lib.tg_bn_grouped_ws_bytes(rows_g, groups, Cc))
    L.check(lib.tg_bn_act_bwd_grouped(_p(dout), _p(y), rows_g, groups, Cc, _p(mean), _p(rstd), _p(gamma.detach()), _p(beta.detach()), act,
                                      slope, _p(dout), _p(dgamma), _p(dbeta), _p(dbias), _p(ws), ws.numel() * 4, _stream()),
            "tg_bn_act_bwd_grouped")
    return dout, dgamma, dbeta, dbias


def bn_running_update_multi(mean, rstd, rows_g, order, running_mean, running_var, nbt, eps=BN_EPS, momentum=BN_MOMENTUM):
    """Running-statistics updates of passes `order` (indices into mean / rstd [groups, C]), one after the other, in ONE launch."""
    arr = (C.c_int * len(order))(*order)
    nbt_p = None if nbt is None else C.c_void_p(nbt.data_ptr())
    L.check(_lib().tg_bn_running_update_multi(_p(mean), _p(rstd), rows_g, mean.shape[-1], eps, momentum, arr, len(order),
                                              _p(running_mean), _p(running_var), nbt_p, _stream()), "tg_bn_running_update_multi")


def bn_act_fwd(y, mean, rstd, gamma, beta, act, slope=0.0, out=None):
    _chk(y, "y"); _chk(out, "out")
    Cc = y.shape[-1]
    if out is None:
        out = torch.empty_like(y)
    L.check(_lib().tg_bn_act_fwd(_p(y), y.numel() // Cc, Cc, _p(mean), _p(rstd), _p(gamma.detach()), _p(beta.detach()), act,
                                 slope, _p(out), _stream()), "tg_bn_act_fwd")
    return out


def bn_act_bwd(dout, y, mean, rstd, gamma, beta, act, slope=0.0, ratio=None, inplace=True, want_dbias=True, outs=None):
    """Returns (dy, dgamma, dbeta, dbias); dy overwrites dout when inplace.  dbias = sum_rows dy (the gradient of
    the bias of the conv feeding this BatchNorm), from the same reduction pass."""
    _chk(dout, "dout"); _chk(y, "y"); _chk(ratio, "ratio")
    Cc = y.shape[-1]
    rows = y.numel() // Cc
    dy = dout if inplace else torch.empty_like(dout)
    if outs is not None:                              # (dgamma, dbeta, dbias) persistent gradient buffers
        dgamma, dbeta, dbias = outs
    else:
        dgamma, dbeta = empty(Cc, like=y), empty(Cc, like=y)
        dbias = empty(Cc, like=y) if want_dbias else None
    lib = _lib()
    ws = workspace(lib.tg_bn_ws_bytes(rows, Cc))
    L.check(lib.tg_bn_act_bwd(_p(dout), _p(y), rows, Cc, _p(mean), _p(rstd), _p(gamma.detach()), _p(beta.detach()), act, slope,
                              _p(ratio), _p(dy), _p(dgamma), _p(dbeta), _p(dbias), _p(ws), ws.numel() * 4, _stream()),
            "tg_bn_act_bwd")
    return dy, dgamma, dbeta, dbias


def bn_bwd_conv1_supported(y_shape):
    Cc = y_shape[-1]
    rows = 1
    for d in y_shape[:-1]:
        rows *= d
    return bool(_lib().tg_bn_bwd_conv1_supported(rows, Cc))


def bn_act_bwd_conv1(dz, w, y, mean, rstd, gamma, beta, act, slope=0.0, ratio=None, want_dbias=True, outs=None):
    """bn_act_bwd with dout = conv_dgrad(dz, w) of a C -> 1 channel 3x3 / stride-1 / pad-1 conv recomputed on the fly from the
    1-channel dz ([B][H][W] or [B][H][W][1]); w = that conv's weight.  Returns (dy, dgamma, dbeta, dbias), dy a new tensor."""
    _chk(dz, "dz"); _chk(y, "y"); _chk(ratio, "ratio")
    wv = weight_view(w)
    _chk(wv, "weight")
    B, H, W, Cc = y.shape
    assert dz.numel() == B * H * W and tuple(wv.shape) == (1, 3, 3, Cc), (tuple(dz.shape), tuple(wv.shape))
    dy = torch.empty_like(y)
    if outs is not None:
        dgamma, dbeta, dbias = outs
    else:
        dgamma, dbeta = empty(Cc, like=y), empty(Cc, like=y)
        dbias = empty(Cc, like=y) if want_dbias else None
    lib = _lib()
    ws = workspace(lib.tg_bn_conv1_ws_bytes(B * H * W, Cc))
    L.check(lib.tg_bn_act_bwd_conv1(_p(dz), _p(wv), B, H, W, _p(y), Cc, _p(mean), _p(rstd), _p(gamma.detach()), _p(beta.detach()), act,
                                    slope, _p(ratio), _p(dy), _p(dgamma), _p(dbeta), _p(dbias), _p(ws), ws.numel() * 4, _stream()),
            "tg_bn_act_bwd_conv1")
    return dy, dgamma, dbeta, dbias


def act_bwd(dout, out, act, slope=0.0, ratio=None, inplace=True):
    _chk(dout, "dout"); _chk(out, "out"); _chk(ratio, "ratio")
    Cc = dout.shape[-1]
    din = dout if inplace else torch.empty_like(dout)
    L.check(_lib().tg_act_bwd(_p(dout), _p(out), dout.numel() // Cc, Cc, act, slope, _p(ratio), _p(din), _stream()), "tg_act_bwd")
    return din


def upcat_bn_supported(up_shape, skip_shape, H, W):
    """Can upcat_fwd(..., up_bn=...) apply the BatchNorm + activation of the layer below while it loads `up`?"""
    B, h, w, Cu = up_shape
    Cs = 0 if skip_shape is None else skip_shape[3]
    return bool(_lib().tg_upcat_bn_supported(B, h, w, Cu, H, W, Cs))


def upcat_fwd(up, skip, H, W, out_mask=None, up_bn=None):
    """up_bn = (mean, rstd, gamma, beta[, act[, slope]]): `up` is a PRE-BatchNorm conv output, act(BN(up)) is formed on load."""
    _chk(up, "up"); _chk(skip, "skip"); _chk(out_mask, "out_mask")
    B, h, w, Cu = up.shape
    Cs = 0 if skip is None else skip.shape[3]
    out = empty(B, H, W, Cu + Cs, like=up)
    if up_bn is not None:
        bn = _bn_act(up_bn)
        L.check(_lib().tg_upcat_fwd_bn(_p(up), C.byref(bn), _p(skip), _p(out_mask), B, h, w, Cu, H, W, Cs, _p(out), _stream()),
                "tg_upcat_fwd_bn")
        return out
    L.check(_lib().tg_upcat_fwd(_p(up), _p(skip), _p(out_mask), B, h, w, Cu, H, W, Cs, _p(out), _stream()), "tg_upcat_fwd")
    return out


def upcat_bwd(dout, h, w, Cu, want_skip=True):
    _chk(dout, "dout")
    B, H, W, Ct = dout.shape
    Cs = Ct - Cu
    dup = empty(B, h, w, Cu, like=dout)
    dskip = empty(B, H, W, Cs, like=dout) if (Cs > 0 and want_skip) else None
    L.check(_lib().tg_upcat_bwd(_p(dout), B, h, w, Cu, H, W, Cs, _p(dup), _p(dskip), _stream()), "tg_upcat_bwd")
    return dup, dskip


def sigmoid_composite_fwd(logits, x, mask, out=None):
    _chk(logits, "logits"); _chk(x, "x"); _chk(mask, "mask"); _chk(out, "out")
    if out is None:
        out = torch.empty_like(x)
    _same_numel(x, "x", logits=logits, mask=mask, out=out)
    L.check(_lib().tg_sigmoid_composite_fwd(_p(logits), _p(x), _p(mask), x.numel(), _p(out), _stream()), "tg_sigmoid_composite_fwd")
    return out


def sigmoid_composite_bwd(dout, logits, mask, want_dx=False):
    _chk(dout, "dout"); _chk(logits, "logits"); _chk(mask, "mask")
    _same_numel(dout, "dout", logits=logits, mask=mask)
    dz = torch.empty_like(logits)
    dx = torch.empty_like(dout) if want_dx else None
    L.check(_lib().tg_sigmoid_composite_bwd(_p(dout), _p(logits), _p(mask), dout.numel(), _p(dz), _p(dx), _stream()),
            "tg_sigmoid_composite_bwd")
    return dz, dx


def maxpool2_fwd(x):
    B, H, W, Cc = x.shape
    out = empty(B, H // 2, W // 2, Cc, like=x)
    L.check(_lib().tg_maxpool2_fwd(_p(x), B, H, W, Cc, _p(out), _stream()), "tg_maxpool2_fwd")
    return out


def maxpool2_bwd(dout, x, relu_gate=False):
    B, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    L.check(_lib().tg_maxpool2_bwd(_p(dout), _p(x), B, H, W, Cc, 1 if relu_gate else 0, _p(dx), _stream()), "tg_maxpool2_bwd")
    return dx


def pixel_losses(pred, target, mask, w_l1, w_tv, w_bnd, l1_weight=None, gscale=None, dpred=None, accumulate=False,
                 want_grad=True, eps=1e-6):
    """-> (out5 device tensor {l1, tv, boundary, sum(band), total}, dpred or None)."""
    _chk(pred, "pred"); _chk(target, "target"); _chk(mask, "mask"); _chk(l1_weight, "l1_weight"); _chk(dpred, "dpred")
    _chk_scalar(gscale, "gscale")
    if pred.dim() != 3:
        raise L.TgError(f"pred: expected [B][H][W], got {tuple(pred.shape)}")
    _same_numel(pred, "pred", target=target, mask=mask, l1_weight=l1_weight, dpred=dpred)
    B, H, W = pred.shape
    out5 = empty(5, like=pred)
    if want_grad and dpred is None:
        dpred = torch.empty_like(pred)
        accumulate = False
    lib = _lib()
    ws = workspace(lib.tg_pixel_loss_ws_bytes(B, H, W))
    L.check(lib.tg_pixel_losses(_p(pred), _p(target), _p(mask), _p(l1_weight), B, H, W, w_l1, w_tv, w_bnd, eps, _p(gscale),
                                _p(out5), _p(dpred) if want_grad else None, 1 if accumulate else 0, _p(ws), ws.numel() * 4,
                                _stream()), "tg_pixel_losses")
    return out5, (dpred if want_grad else None)


def l1_mean(a, b, coef=1.0, gscale=None, want_grad=True, relu_gate=False):
    """relu_gate: `a` is a ReLU output; the gradient returned is the one in front of that ReLU (zero where a <= 0)."""
    _chk(a, "a"); _chk(b, "b")
    out = empty(1, like=a)
    da = torch.empty_like(a) if want_grad else None
    lib = _lib()
    ws = workspace(lib.tg_reduce_ws_bytes(a.numel()))
    fn = lib.tg_l1_mean_relu if relu_gate else lib.tg_l1_mean
    L.check(fn(_p(a), _p(b), a.numel(), coef, _p(gscale), _p(out), _p(da), _p(ws), ws.numel() * 4, _stream()), "tg_l1_mean")
    return out, da


def bce_logits(z, target, coef=1.0, gscale=None, want_grad=True, dz_out=None):
    """dz_out: preallocated destination of the gradient (a slice of a stacked buffer), same shape as z."""
    _chk(z, "z"); _chk(dz_out, "dz_out")
    out = empty(1, like=z)
    if dz_out is not None:
        assert want_grad and dz_out.shape == z.shape
    dz = (dz_out if dz_out is not None else torch.empty_like(z)) if want_grad else None
    lib = _lib()
    ws = workspace(lib.tg_reduce_ws_bytes(z.numel()))
    L.check(lib.tg_bce_logits(_p(z), z.numel(), target, coef, _p(gscale), _p(out), _p(dz), _p(ws), ws.numel() * 4, _stream()),
            "tg_bce_logits")
    return out, dz


QUALITY_KEYS = ("mse", "psnr", "ssim", "l1_distance", "l2_distance", "boundary_mse", "boundary_psnr",
                "boundary_gradient_diff", "boundary_sum")


def quality_metrics(pred, target, mask):
    """-> 9-element device tensor, QUALITY_KEYS order (tg_quality_metrics); pred/target/mask [B,1,H,W] or [B,H,W]."""
    _chk(pred, "pred"); _chk(target, "target"); _chk(mask, "mask")
    H, W = pred.shape[-2], pred.shape[-1]
    imgs = pred.numel() // (H * W)
    assert target.shape == pred.shape and mask.numel() == pred.numel(), (pred.shape, target.shape, mask.shape)
    out = empty(9, like=pred)
    lib = _lib()
    ws = workspace(lib.tg_quality_metrics_ws_bytes(imgs, H, W))
    L.check(lib.tg_quality_metrics(_p(pred), _p(target), _p(mask), imgs, H, W, _p(out), _p(ws), ws.numel() * 4, _stream()),
            "tg_quality_metrics")
    return out


def u8_to_tiles(img_u8=None, mask_u8=None):
    """uint8 device tensors -> (image/255, mask>0) fp32 device tensors of the same shape (tg_u8_to_tiles)."""
    ref = img_u8 if img_u8 is not None else mask_u8
    for t in (img_u8, mask_u8):
        if t is not None and (not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous()):
            raise L.TgError("u8_to_tiles: expected contiguous uint8 HIP tensors")
    img = torch.empty(ref.shape, dtype=torch.float32, device=ref.device) if img_u8 is not None else None
    msk = torch.empty(ref.shape, dtype=torch.float32, device=ref.device) if mask_u8 is not None else None
    L.check(_lib().tg_u8_to_tiles(_p(img_u8), _p(mask_u8), ref.numel(), _p(img), _p(msk), _stream()), "tg_u8_to_tiles")
    return img, msk


def raster_plan(H, W, wh, ww, overlap, ny, nx):
    return L.TgRasterPlan(H, W, wh, ww, overlap, ny, nx)


def _raster_in(dem, mask, plan):
    _chk(dem, "dem"); _chk(mask, "mask")
    if tuple(dem.shape) != (plan.H, plan.W) or (mask is not None and tuple(mask.shape) != (plan.H, plan.W)):
        raise L.TgError(f"raster: dem {tuple(dem.shape)} / mask {None if mask is None else tuple(mask.shape)} "
                        f"differ from the plan's {plan.H}x{plan.W}")


def _i32(t, n, name):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n):
        raise L.TgError(f"{name}: expected a contiguous int32 HIP tensor of {n} elements")


def raster_window_stats(dem, mask, plan, nodata=None):
    """-> (lo [nwin], hi [nwin], counts int32 [nwin][2] = known, holes) over the windows of `plan` (tg_raster_window_stats)."""
    _raster_in(dem, mask, plan)
    nwin = plan.ny * plan.nx
    lo, hi = empty(nwin, like=dem), empty(nwin, like=dem)
    counts = torch.empty(nwin, 2, dtype=torch.int32, device=dem.device)
    L.check(_lib().tg_raster_window_stats(_p(dem), _p(mask), C.byref(plan), int(nodata is not None),
                                          0.0 if nodata is None else float(nodata), _p(lo), _p(hi), _p(counts), _stream()),
            "tg_raster_window_stats")
    return lo, hi, counts


def raster_gather(dem, mask, plan, lo, hi, win_idx, nodata=None, x=None, m=None):
    """Normalised network input and mask [n][wh][ww] of the windows win_idx (int32 HIP tensor) (tg_raster_gather)."""
    _raster_in(dem, mask, plan)
    n, nwin = win_idx.numel(), plan.ny * plan.nx
    _i32(win_idx, n, "win_idx")
    _chk(lo, "lo"); _chk(hi, "hi")
    assert lo.numel() == nwin and hi.numel() == nwin, (lo.shape, hi.shape, nwin)
    shape = (n, plan.wh, plan.ww)
    x = empty(*shape, like=dem) if x is None else x
    m = empty(*shape, like=dem) if m is None else m
    for t, nm in ((x, "x"), (m, "m")):
        _chk(t, nm)
        if tuple(t.shape) != shape:
            raise L.TgError(f"raster_gather: {nm} {tuple(t.shape)} != {shape}")
    L.check(_lib().tg_raster_gather(_p(dem), _p(mask), C.byref(plan), int(nodata is not None),
                                    0.0 if nodata is None else float(nodata), _p(lo), _p(hi), _p(win_idx), n, _p(x), _p(m),
                                    _stream()), "tg_raster_gather")
    return x, m


def raster_blend(dem, mask, plan, lo, hi, run_of_window, wout, nodata=None):
    """-> (raster [H][W], unfilled int32 [1] device counter) (tg_raster_blend).  run_of_window: int32 [nwin], the row of
    wout [n_run][wh][ww] holding that window's generator output, -1 where it did not run."""
    _raster_in(dem, mask, plan)
    nwin = plan.ny * plan.nx
    _i32(run_of_window, nwin, "run_of_window")
    _chk(lo, "lo"); _chk(hi, "hi"); _chk(wout, "wout")
    assert lo.numel() == nwin and hi.numel() == nwin, (lo.shape, hi.shape, nwin)
    if wout.dim() != 3 or tuple(wout.shape[1:]) != (plan.wh, plan.ww):
        raise L.TgError(f"raster_blend: wout {tuple(wout.shape)} is not [n_run][{plan.wh}][{plan.ww}]")
    out = empty(plan.H, plan.W, like=dem)
    unfilled = torch.empty(1, dtype=torch.int32, device=dem.device)
    L.check(_lib().tg_raster_blend(_p(dem), _p(mask), C.byref(plan), int(nodata is not None),
                                   0.0 if nodata is None else float(nodata), _p(lo), _p(hi), _p(run_of_window),
                                   _p(wout) if wout.numel() else None, wout.shape[0], _p(out), _p(unfilled), _stream()),
            "tg_raster_blend")
    return out, unfilled


def _host_ops(ops, n, name):
    """The transforms of a call as a host int32 array of n entries (the library reads and checks them before any launch)."""
    a = np.ascontiguousarray(ops.cpu().numpy() if isinstance(ops, torch.Tensor) else ops)
    if a.ndim != 1 or a.size != n or a.dtype.kind not in "iu":
        raise L.TgError(f"{name}: expected {n} integer transforms on the host, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a, dtype=np.int32)


def raster_gather_ops(dem, mask, plan, lo, hi, win_idx, op_idx, nodata=None, x=None, m=None):
    """raster_gather with a transform per list item: item k is window win_idx[k] (int32 HIP tensor) under op_idx[k] (host
    integers, 0..7 as in raster_sample), written in the member's frame [n][wh][ww] (tg_raster_gather_ops)."""
    _raster_in(dem, mask, plan)
    n, nwin = win_idx.numel(), plan.ny * plan.nx
    _i32(win_idx, n, "win_idx")
    op_idx = _host_ops(op_idx, n, "raster_gather_ops")
    _chk(lo, "lo"); _chk(hi, "hi")
    assert lo.numel() == nwin and hi.numel() == nwin, (lo.shape, hi.shape, nwin)
    shape = (n, plan.wh, plan.ww)
    x = empty(*shape, like=dem) if x is None else x
    m = empty(*shape, like=dem) if m is None else m
    for t, nm in ((x, "x"), (m, "m")):
        _chk(t, nm)
        if tuple(t.shape) != shape:
            raise L.TgError(f"raster_gather_ops: {nm} {tuple(t.shape)} != {shape}")
    L.check(_lib().tg_raster_gather_ops(_p(dem), _p(mask), C.byref(plan), int(nodata is not None),
                                        0.0 if nodata is None else float(nodata), _p(lo), _p(hi), _p(win_idx),
                                        op_idx.ctypes.data, n, _p(x), _p(m), _stream()), "tg_raster_gather_ops")
    return x, m


def raster_tta_reduce(gout, ops, mean=None, var=None):
    """gout [n][T][wh][ww]: generator outputs of n windows under the transforms ops (T host integers, T = 2, 4 or 8), each in
    its member frame -> (mean, var) [n][wh][ww] in the windows' frame, the sample variance over T - 1 (tg_raster_tta_reduce)."""
    _chk(gout, "gout")
    if gout.dim() != 4:
        raise L.TgError(f"raster_tta_reduce: gout {tuple(gout.shape)} is not [n][T][wh][ww]")
    n, T, wh, ww = gout.shape
    ops = _host_ops(ops, T, "raster_tta_reduce")
    mean = empty(n, wh, ww, like=gout) if mean is None else mean
    var = empty(n, wh, ww, like=gout) if var is None else var
    for t, nm in ((mean, "mean"), (var, "var")):
        _chk(t, nm)
        if tuple(t.shape) != (n, wh, ww):
            raise L.TgError(f"raster_tta_reduce: {nm} {tuple(t.shape)} != {(n, wh, ww)}")
    L.check(_lib().tg_raster_tta_reduce(_p(gout), ops.ctypes.data, T, n, wh, ww, _p(mean), _p(var), _stream()),
            "tg_raster_tta_reduce")
    return mean, var


def raster_blend_tta(dem, mask, plan, lo, hi, run_of_window, wmean, wvar, nodata=None):
    """raster_blend of the window means wmean plus the spread map -> (raster [H][W], spread [H][W] in metres: 0 at known pixels,
    NaN where no running window covers a hole, unfilled int32 [1] device counter) (tg_raster_blend_tta).  wmean, wvar:
    [n_run][wh][ww], raster_tta_reduce's outputs in the rows run_of_window names."""
    _raster_in(dem, mask, plan)
    nwin = plan.ny * plan.nx
    _i32(run_of_window, nwin, "run_of_window")
    _chk(lo, "lo"); _chk(hi, "hi"); _chk(wmean, "wmean"); _chk(wvar, "wvar")
    assert lo.numel() == nwin and hi.numel() == nwin, (lo.shape, hi.shape, nwin)
    if wmean.dim() != 3 or tuple(wmean.shape[1:]) != (plan.wh, plan.ww) or wvar.shape != wmean.shape:
        raise L.TgError(f"raster_blend_tta: wmean {tuple(wmean.shape)} / wvar {tuple(wvar.shape)} are not "
                        f"[n_run][{plan.wh}][{plan.ww}]")
    out, spread = empty(plan.H, plan.W, like=dem), empty(plan.H, plan.W, like=dem)
    unfilled = torch.empty(1, dtype=torch.int32, device=dem.device)
    some = wmean.numel() > 0
    L.check(_lib().tg_raster_blend_tta(_p(dem), _p(mask), C.byref(plan), int(nodata is not None),
                                       0.0 if nodata is None else float(nodata), _p(lo), _p(hi), _p(run_of_window),
                                       _p(wmean) if some else None, _p(wvar) if some else None, wmean.shape[0], _p(out),
                                       _p(spread), _p(unfilled), _stream()), "tg_raster_blend_tta")
    return out, spread, unfilled


HOLE_RECT, HOLE_ELLIPSE, HOLE_STROKE = 0, 1, 2    # primitive kinds of tg_hole_masks (terragan_hip.h)


def _i32_rows(t, cols, name):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == cols):
        raise L.TgError(f"{name}: expected a contiguous int32 HIP tensor [n][{cols}], got {t.dtype} {tuple(t.shape)} on {t.device}")


def hole_masks(prims, offsets, side, out=None):
    """Hole masks [n][side][side] (1 = keep, 0 = hole) from int32 primitives prims [P][8] and offsets [n+1] (tg_hole_masks).
    offsets must be nondecreasing from 0 to P with at most 32 primitives per window: the caller's contract, not checked
    here (that would need a host sync)."""
    _i32_rows(prims, 8, "prims")
    if not (offsets.is_cuda and offsets.dtype == torch.int32 and offsets.is_contiguous() and offsets.dim() == 1
            and offsets.numel() >= 2):
        raise L.TgError("offsets: expected a contiguous int32 HIP tensor [n+1], n >= 1")
    n = offsets.numel() - 1
    shape = (n, side, side)
    out = torch.empty(shape, dtype=torch.float32, device=offsets.device) if out is None else out
    _chk(out, "out")
    if tuple(out.shape) != shape:
        raise L.TgError(f"hole_masks: out {tuple(out.shape)} != {shape}")
    # an empty primitive list has no storage; any non-null pointer does, since no window then reads a primitive
    L.check(_lib().tg_hole_masks(_p(prims) if prims.numel() else _p(offsets), _p(offsets), n, int(side), _p(out), _stream()),
            "tg_hole_masks")
    return out


def raster_sample(dem, draws, mask, norm_known=True, x=None, lo=None, hi=None):
    """Windows of dem [H][W] at draws int32 [n][3] = (y0, x0, op), normalised by the min / max over mask != 0 (norm_known)
    or over all pixels (tg_raster_sample).  mask: [n][side][side].  -> (x [n][side][side], lo [n], hi [n])."""
    _chk(dem, "dem"); _chk(mask, "mask")
    _i32_rows(draws, 3, "draws")
    if dem.dim() != 2:
        raise L.TgError(f"raster_sample: dem must be [H][W], got {tuple(dem.shape)}")
    n = draws.shape[0]
    if mask.dim() != 3 or mask.shape[0] != n or mask.shape[1] != mask.shape[2]:
        raise L.TgError(f"raster_sample: mask {tuple(mask.shape)} is not [{n}][side][side]")
    side = mask.shape[1]
    x = empty(n, side, side, like=dem) if x is None else x
    lo = empty(n, like=dem) if lo is None else lo
    hi = empty(n, like=dem) if hi is None else hi
    for t, nm, shp in ((x, "x", (n, side, side)), (lo, "lo", (n,)), (hi, "hi", (n,))):
        _chk(t, nm)
        if tuple(t.shape) != shp:
            raise L.TgError(f"raster_sample: {nm} {tuple(t.shape)} != {shp}")
    L.check(_lib().tg_raster_sample(_p(dem), dem.shape[0], dem.shape[1], _p(draws), n, side, _p(mask), int(bool(norm_known)),
                                    _p(x), _p(lo), _p(hi), _stream()), "tg_raster_sample")
    return x, lo, hi


MORPH_ERODE, MORPH_DILATE = 0, 1                  # tg_objmask_morph ops (terragan_hip.h)
OBJMASK_MAX_BUFFER = 64


def _hip(t, dtype, shape, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape):
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise L.TgError(f"{name}: expected a contiguous {dtype} HIP tensor {list(shape)}, got {got}")


def _raster_hw(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise L.TgError(f"{name}: expected a [H][W] tensor")
    H, W = t.shape
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise L.TgError(f"{name}: raster {H}x{W} must be non-empty with H*W < 2^31 (int32 labels)")
    return int(H), int(W)


def _radius(r, H, W):
    r = int(r)
    if r < 0:
        raise L.TgError(f"objmask: radius {r} < 0")
    return min(r, max(H, W))             # a window past the raster is the raster: the same result


def objmask_known(dem, mask=None, nodata=None, transposed=True):
    """-> (known uint8 [H][W], known_t uint8 [W][H] or None): mask != 0, finite and != nodata (tg_objmask_known)."""
    H, W = _raster_hw(dem, "dem")
    _hip(dem, torch.float32, (H, W), "dem")
    if mask is not None:
        _hip(mask, torch.float32, (H, W), "mask")
    known = torch.empty(H, W, dtype=torch.uint8, device=dem.device)
    known_t = torch.empty(W, H, dtype=torch.uint8, device=dem.device) if transposed else None
    L.check(_lib().tg_objmask_known(_p(dem), _p(mask), H, W, int(nodata is not None), 0.0 if nodata is None else float(nodata),
                                    _p(known), _p(known_t), _stream()), "tg_objmask_known")
    return known, known_t


def objmask_morph(x, radius, op, known=None):
    """Clipped-window erosion (op MORPH_ERODE) or dilation (MORPH_DILATE) of x [H][W] over the pixels with known != 0
    (every pixel when known is None) (tg_objmask_morph)."""
    H, W = _raster_hw(x, "x")
    _hip(x, torch.float32, (H, W), "x")
    if known is not None:
        _hip(known, torch.uint8, (H, W), "known")
    if op not in (MORPH_ERODE, MORPH_DILATE):
        raise L.TgError(f"objmask_morph: op {op} is neither MORPH_ERODE nor MORPH_DILATE")
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    L.check(_lib().tg_objmask_morph(_p(x), _p(known), H, W, _radius(radius, H, W), int(op), _p(tmp), _p(out), _stream()),
            "tg_objmask_morph")
    return out


def objmask_pmf_step(s, known, known_t, radius, dh, flags, t0, t1, out):
    """out = open_r(s) over the known pixels; flags |= known & (s - out > dh) (tg_objmask_pmf_step).  t0, t1: scratch."""
    H, W = _raster_hw(s, "s")
    for t, nm in ((s, "s"), (t0, "t0"), (t1, "t1"), (out, "out")):
        _hip(t, torch.float32, (H, W), nm)
    _hip(known, torch.uint8, (H, W), "known")
    _hip(known_t, torch.uint8, (W, H), "known_t")
    _hip(flags, torch.uint8, (H, W), "flags")
    L.check(_lib().tg_objmask_pmf_step(_p(s), _p(known), _p(known_t), H, W, _radius(radius, H, W), float(dh), _p(t0), _p(t1),
                                       _p(out), _p(flags), _stream()), "tg_objmask_pmf_step")
    return out


def objmask_components(flags):
    """-> (labels int32 [H][W]: smallest linear index of the 8-connected component, -1 off the flags; area int32 [H*W]: the
    component size at that index) (tg_objmask_components)."""
    H, W = _raster_hw(flags, "flags")
    _hip(flags, torch.uint8, (H, W), "flags")
    labels = torch.empty(H, W, dtype=torch.int32, device=flags.device)
    area = torch.empty(H * W, dtype=torch.int32, device=flags.device)
    L.check(_lib().tg_objmask_components(_p(flags), H, W, _p(labels), _p(area), _stream()), "tg_objmask_components")
    return labels, area


def objmask_filter(known, labels, area, min_area, buffer_px):
    """-> (objects uint8 [H][W], keep float32 [H][W], counts int32 [4] = flagged, kept, removed, object pixels)
    (tg_objmask_filter)."""
    H, W = _raster_hw(known, "known")
    _hip(known, torch.uint8, (H, W), "known")
    _hip(labels, torch.int32, (H, W), "labels")
    _hip(area, torch.int32, (H * W,), "area")
    if not 0 <= int(min_area) < 2 ** 31:
        raise L.TgError(f"objmask_filter: min_area {min_area} out of range [0, 2^31)")
    if not 0 <= int(buffer_px) <= OBJMASK_MAX_BUFFER:
        raise L.TgError(f"objmask_filter: buffer {buffer_px} px out of range [0, {OBJMASK_MAX_BUFFER}]")
    objects = torch.empty(H, W, dtype=torch.uint8, device=known.device)
    keep = torch.empty(H, W, dtype=torch.float32, device=known.device)
    counts = torch.empty(4, dtype=torch.int32, device=known.device)
    L.check(_lib().tg_objmask_filter(_p(known), _p(labels), _p(area), H, W, int(min_area), int(buffer_px), _p(objects), _p(keep),
                                     _p(counts), _stream()), "tg_objmask_filter")
    return objects, keep, counts


HOLE_COLS = 9                                     # tg_hole_table rows: label, area, scored, sum, max bits, y0, x0, y1, x1
TE_NSUM, TE_NCOUNT, SELECT_MAX_K = 10 + 2 * L.TG_EVAL_MAX_CLASSES, 10, 8


def eval_holes(dem, mask, nodata, objects, cell_masks, cell_of, tile, row0, row1, holes, keep, counts, hole_in=None):
    """Evaluation holes of raster rows [row0, row1) into holes uint8 / keep float32 [H][W]; counts int64 [3] (valid, holes,
    valid object pixels) are added to (tg_eval_holes).  cell_masks [n][tile][tile] / cell_of int32 [ncy][ncx] may be None."""
    H, W = _raster_hw(dem, "dem")
    _hip(dem, torch.float32, (H, W), "dem")
    if mask is not None:
        _hip(mask, torch.float32, (H, W), "mask")
    if objects is not None:
        _hip(objects, torch.uint8, (H, W), "objects")
    if hole_in is not None:
        _hip(hole_in, torch.uint8, (H, W), "hole_in")
    if cell_of is not None:
        _hip(cell_of, torch.int32, (-(-H // tile), -(-W // tile)), "cell_of")
        if cell_masks is None or cell_masks.dim() != 3:
            raise L.TgError("eval_holes: cell_of needs cell_masks [n][tile][tile]")
        _hip(cell_masks, torch.float32, (cell_masks.shape[0], tile, tile), "cell_masks")
    _hip(holes, torch.uint8, (H, W), "holes")
    _hip(keep, torch.float32, (H, W), "keep")
    _hip(counts, torch.int64, (3,), "counts")
    L.check(_lib().tg_eval_holes(_p(dem), _p(mask), int(nodata is not None), 0.0 if nodata is None else float(nodata),
                                 _p(objects), _p(cell_masks) if cell_of is not None else None, _p(cell_of), _p(hole_in), H, W,
                                 int(tile), int(row0), int(row1), _p(holes), _p(keep), _p(counts), _stream()), "tg_eval_holes")


def hole_table(labels, area, cap, slot=None):
    """-> (table int64 [cap][HOLE_COLS], slot int32 [H*W], count int32 [1]) (tg_hole_table).  slot may be `area` itself."""
    H, W = _raster_hw(labels, "labels")
    _hip(labels, torch.int32, (H, W), "labels")
    _hip(area, torch.int32, (H * W,), "area")
    slot = torch.empty(H * W, dtype=torch.int32, device=labels.device) if slot is None else slot
    _hip(slot, torch.int32, (H * W,), "slot")
    if not 0 <= int(cap) < 2 ** 31:
        raise L.TgError(f"hole_table: cap {cap} out of range [0, 2^31)")
    table = torch.empty(max(int(cap), 1), HOLE_COLS, dtype=torch.int64, device=labels.device)
    count = torch.empty(1, dtype=torch.int32, device=labels.device)
    L.check(_lib().tg_hole_table(_p(labels), _p(area), H, W, _p(slot), _p(table), int(cap), _p(count), _stream()),
            "tg_hole_table")
    return table[:int(cap)], slot, count


def terrain_errors(z, p, mask, nodata, holes, keep, labels, slot, table, cellsize, class_px):
    """-> (sums float64 [TE_NSUM], counts int64 [TE_NCOUNT], sel_a [H*W], sel_slope [H*W]) (tg_terrain_errors and
    tg_terrain_errors_finish).  table: the rows of hole_table; class_px: the class edges in pixels."""
    H, W = _raster_hw(z, "z")
    for t, nm in ((z, "z"), (p, "p"), (keep, "keep")):
        _hip(t, torch.float32, (H, W), nm)
    if mask is not None:
        _hip(mask, torch.float32, (H, W), "mask")
    _hip(holes, torch.uint8, (H, W), "holes")
    _hip(labels, torch.int32, (H, W), "labels")
    _hip(slot, torch.int32, (H * W,), "slot")
    _hip(table, torch.int64, (table.shape[0], HOLE_COLS), "table")
    if len(class_px) > L.TG_EVAL_MAX_CLASSES - 1:
        raise L.TgError(f"terrain_errors: {len(class_px)} class edges, at most {L.TG_EVAL_MAX_CLASSES - 1}")
    cls = L.TgAreaClasses(len(class_px), 0)
    for j, v in enumerate(class_px):
        cls.px[j] = int(v)
    lib = _lib()
    dev = z.device
    counts = torch.empty(TE_NCOUNT, dtype=torch.int64, device=dev)
    sel_a = torch.empty(H * W, dtype=torch.float32, device=dev)
    sel_s = torch.empty(H * W, dtype=torch.float32, device=dev)
    sums = torch.empty(TE_NSUM, dtype=torch.float64, device=dev)
    nb = lib.tg_terrain_errors_ws_bytes(H, W)
    ws = workspace(nb)
    L.check(lib.tg_terrain_errors(_p(z), _p(p), _p(mask), int(nodata is not None), 0.0 if nodata is None else float(nodata),
                                  _p(holes), _p(keep), _p(labels), _p(slot), _p(table) if table.numel() else None,
                                  table.shape[0], H, W, float(cellsize), C.byref(cls), _p(counts), _p(sel_a), _p(sel_s),
                                  _p(ws), ws.numel() * 4, _stream()), "tg_terrain_errors")
    L.check(lib.tg_terrain_errors_finish(H, W, _p(ws), ws.numel() * 4, _p(sums), _stream()), "tg_terrain_errors_finish")
    return sums, counts, sel_a, sel_s


def select_f32(v, ks):
    """-> float32 [len(ks)]: the ks[j]-th smallest of the non-NaN, non-negative values of v, NaN for k out of range
    (tg_select_f32)."""
    if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
        raise L.TgError("select_f32: expected a contiguous float32 HIP tensor")
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= SELECT_MAX_K:
        raise L.TgError(f"select_f32: {len(ks)} ranks, expected 1 .. {SELECT_MAX_K}")
    kd = torch.tensor(ks, dtype=torch.int64).to(v.device)
    out = torch.empty(len(ks), dtype=torch.float32, device=v.device)
    lib = _lib()
    ws = workspace(lib.tg_select_f32_ws_bytes(v.numel(), len(ks)))
    L.check(lib.tg_select_f32(_p(v), v.numel(), _p(kd), len(ks), _p(out), _p(ws), ws.numel() * 4, _stream()), "tg_select_f32")
    return out


EDT_FAR, EDT_MAX_SIDE, DEPTH_MAX_CLASSES = L.TG_EDT_FAR, L.TG_EDT_MAX_SIDE, L.TG_DEPTH_MAX_CLASSES


def _edt_hw(t, name):
    H, W = _raster_hw(t, name)
    if max(H, W) > EDT_MAX_SIDE:
        raise L.TgError(f"{name}: raster {H}x{W}: both sides must be at most {EDT_MAX_SIDE} (int32 squared distances)")
    return H, W


def edt(seed, cap2=0, cellsize=None):
    """-> (d2 int32 [H][W], dist_m float32 [H][W] or None): d2 = min(exact squared Euclidean distance in pixels to the nearest
    nonzero pixel of seed uint8 [H][W], cap2), EDT_FAR without a seed and without a cap (cap2 <= 0); dist_m =
    cellsize * sqrt(d2) with a cellsize (tg_edt)."""
    H, W = _edt_hw(seed, "seed")
    _hip(seed, torch.uint8, (H, W), "seed")
    cap2 = int(cap2)
    if not -2 ** 31 <= cap2 < 2 ** 31:
        raise L.TgError(f"edt: cap2 {cap2} does not fit an int32")
    c = 0.0
    if cellsize is not None:
        c = float(cellsize)
        if not (c > 0 and c < float("inf")):
            raise L.TgError(f"edt: cellsize {cellsize!r} must be finite and > 0")
    d2 = torch.empty(H, W, dtype=torch.int32, device=seed.device)
    dist = torch.empty(H, W, dtype=torch.float32, device=seed.device) if cellsize is not None else None
    lib = _lib()
    ws = workspace(lib.tg_edt_ws_bytes(H, W))
    L.check(lib.tg_edt(_p(seed), H, W, cap2, c, _p(d2), _p(dist), _p(ws), ws.numel() * 4, _stream()), "tg_edt")
    return d2, dist


def depth_errors(sel_a, d2, labels, slot, nholes, class_d2):
    """-> (sums float64 [2 * DEPTH_MAX_CLASSES]: sum a, sum a^2 per class; counts int64 [DEPTH_MAX_CLASSES]; max_bits uint32 as
    int32 [DEPTH_MAX_CLASSES]; hole_d2 int32 [nholes]: the largest d2 of each hole) (tg_depth_errors and
    tg_depth_errors_finish).  sel_a [H*W]: terrain_errors' |error| on the scored pixels, NaN elsewhere; class_d2: the class
    edges as squared pixel distances, nondecreasing."""
    H, W = _edt_hw(d2, "d2")
    _hip(d2, torch.int32, (H, W), "d2")
    _hip(sel_a, torch.float32, (H * W,), "sel_a")
    _hip(labels, torch.int32, (H, W), "labels")
    _hip(slot, torch.int32, (H * W,), "slot")
    nholes = int(nholes)
    if not 0 <= nholes < 2 ** 31:
        raise L.TgError(f"depth_errors: nholes {nholes} out of range [0, 2^31)")
    edges = [int(v) for v in class_d2]
    if len(edges) > DEPTH_MAX_CLASSES - 1 or any(not 0 <= v < 2 ** 31 for v in edges) or edges != sorted(edges):
        raise L.TgError(f"depth_errors: class edges {edges} must be at most {DEPTH_MAX_CLASSES - 1} nondecreasing int32 values "
                        ">= 0")
    cls = L.TgDepthClasses(len(edges), 0)
    for j, v in enumerate(edges):
        cls.d2[j] = v
    lib = _lib()
    dev = d2.device
    counts = torch.empty(DEPTH_MAX_CLASSES, dtype=torch.int64, device=dev)
    max_bits = torch.empty(DEPTH_MAX_CLASSES, dtype=torch.int32, device=dev)
    hole_d2 = torch.empty(nholes, dtype=torch.int32, device=dev)
    sums = torch.empty(2 * DEPTH_MAX_CLASSES, dtype=torch.float64, device=dev)
    ws = workspace(lib.tg_depth_errors_ws_bytes(H, W))
    L.check(lib.tg_depth_errors(_p(sel_a), _p(d2), _p(labels), _p(slot), nholes, H, W, C.byref(cls), _p(counts), _p(max_bits),
                                _p(hole_d2) if nholes else None, _p(ws), ws.numel() * 4, _stream()), "tg_depth_errors")
    L.check(lib.tg_depth_errors_finish(H, W, _p(ws), ws.numel() * 4, _p(sums), _stream()), "tg_depth_errors_finish")
    return sums, counts, max_bits, hole_d2


def edt_nearest(seed, cap2=0):
    """-> (d2 int32 [H][W], idx int32 [H][W]): d2 as edt's; idx = y * W + x of the nearest nonzero pixel of seed (the smallest
    row, then the smallest column among equals), -1 where d2 is EDT_FAR or, with a cap, d2 >= cap2 (tg_edt_nearest)."""
    H, W = _edt_hw(seed, "seed")
    _hip(seed, torch.uint8, (H, W), "seed")
    cap2 = int(cap2)
    if not -2 ** 31 <= cap2 < 2 ** 31:
        raise L.TgError(f"edt_nearest: cap2 {cap2} does not fit an int32")
    d2 = torch.empty(H, W, dtype=torch.int32, device=seed.device)
    idx = torch.empty(H, W, dtype=torch.int32, device=seed.device)
    lib = _lib()
    ws = workspace(lib.tg_edt_nearest_ws_bytes(H, W))
    L.check(lib.tg_edt_nearest(_p(seed), H, W, cap2, _p(d2), _p(idx), _p(ws), ws.numel() * 4, _stream()), "tg_edt_nearest")
    return d2, idx


def rayfill(z, known, lim2=0, power=2.0, d2=None, idx=None, want_hits=False):
    """-> (out float32 [H][W], counts int64 [3]: by rays, by nearest, left NaN; hits uint16 [8][H][W] or None): the
    eight-direction inverse-distance fill of the pixels with known == 0 (tg_rayfill).  d2, idx: edt_nearest's, for the
    nearest-neighbour fallback of the pixels no ray serves; both or neither."""
    H, W = _edt_hw(z, "z")
    _hip(z, torch.float32, (H, W), "z")
    _hip(known, torch.uint8, (H, W), "known")
    lim2 = int(lim2)
    if not -2 ** 31 <= lim2 < 2 ** 31:
        raise L.TgError(f"rayfill: lim2 {lim2} does not fit an int32")
    power = float(power)
    if not 0.0 < power <= 8.0:
        raise L.TgError(f"rayfill: power {power!r} must lie in (0, 8]")
    if (d2 is None) != (idx is None):
        raise L.TgError("rayfill: d2 and idx go together")
    if d2 is not None:
        _hip(d2, torch.int32, (H, W), "d2")
        _hip(idx, torch.int32, (H, W), "idx")
    out = torch.empty(H, W, dtype=torch.float32, device=z.device)
    hits = torch.empty(8, H, W, dtype=torch.uint16, device=z.device) if want_hits else None
    counts = torch.empty(3, dtype=torch.int64, device=z.device)
    lib = _lib()
    ws = workspace(lib.tg_rayfill_ws_bytes(H, W))
    L.check(lib.tg_rayfill(_p(z), _p(known), H, W, lim2, power, _p(d2), _p(idx), _p(out), _p(hits), _p(counts), _p(ws),
                           ws.numel() * 4, _stream()), "tg_rayfill")
    return out, counts, hits


def gather_fill(z, known, idx):
    """-> (out float32 [H][W] = known ? z : z[idx], NaN at idx < 0; counts int64 [2]: filled, left NaN) (tg_gather_fill)."""
    H, W = _edt_hw(z, "z")
    _hip(z, torch.float32, (H, W), "z")
    _hip(known, torch.uint8, (H, W), "known")
    _hip(idx, torch.int32, (H, W), "idx")
    out = torch.empty(H, W, dtype=torch.float32, device=z.device)
    counts = torch.empty(2, dtype=torch.int64, device=z.device)
    L.check(_lib().tg_gather_fill(_p(z), _p(known), _p(idx), H, W, _p(out), _p(counts), _stream()), "tg_gather_fill")
    return out, counts


NATURAL_MAX_RADIUS = 32
NATURAL_TILE = (4, 64)                                    # natural.hip's NAT_TH, NAT_TW


def _natural_radius(radius, who):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= NATURAL_MAX_RADIUS:
        raise L.TgError(f"{who}: radius {radius!r} must be an integer in [1, {NATURAL_MAX_RADIUS}]")
    return int(radius)


def natural_tile_maxima(d2, radius=32):
    """-> uint16 [ceil(H / 4)][ceil(W / 64)]: the largest c = min(d2, radius^2) of every tile of NATURAL_TILE pixels
    (tg_natural_tile_maxima): the pre-pass of natural_fill on its own."""
    H, W = _edt_hw(d2, "d2")
    _hip(d2, torch.int32, (H, W), "d2")
    radius = _natural_radius(radius, "natural_tile_maxima")
    lib = _lib()
    th, tw = NATURAL_TILE
    nty, ntx = -(-H // th), -(-W // tw)
    nbytes = lib.tg_natural_fill_ws_bytes(H, W)
    ws = torch.empty(nbytes // 2, dtype=torch.uint16, device=d2.device)
    L.check(lib.tg_natural_tile_maxima(_p(d2), H, W, radius, _p(ws), nbytes, _stream()), "tg_natural_tile_maxima")
    return ws[:nty * ntx].view(nty, ntx)


def natural_fill(nn, d2, known, radius=32, lim2=0, want_support=False):
    """-> (out float32 [H][W], counts int64 [2]: void pixels filled, left NaN; support int32 [H][W] or None): the discrete
    Sibson (natural-neighbour) fill of the pixels with known == 0 (tg_natural_fill).  nn: gather_fill's nearest fill; d2:
    edt_nearest's squared distances WITHOUT a cap; a void pixel farther than lim2 (> 0) from every known pixel is NaN."""
    H, W = _edt_hw(nn, "nn")
    _hip(nn, torch.float32, (H, W), "nn")
    _hip(d2, torch.int32, (H, W), "d2")
    _hip(known, torch.uint8, (H, W), "known")
    radius = _natural_radius(radius, "natural_fill")
    lim2 = int(lim2)
    if not -2 ** 31 <= lim2 < 2 ** 31:
        raise L.TgError(f"natural_fill: lim2 {lim2} does not fit an int32")
    out = torch.empty(H, W, dtype=torch.float32, device=nn.device)
    support = torch.empty(H, W, dtype=torch.int32, device=nn.device) if want_support else None
    counts = torch.empty(2, dtype=torch.int64, device=nn.device)
    lib = _lib()
    ws = workspace(lib.tg_natural_fill_ws_bytes(H, W))
    L.check(lib.tg_natural_fill(_p(nn), _p(d2), _p(known), H, W, radius, lim2, _p(out), _p(support), _p(counts), _p(ws),
                                ws.numel() * 4, _stream()), "tg_natural_fill")
    return out, counts, support


def void_smooth(x, known, steps=1):
    """-> float32 [H][W]: `steps` Jacobi steps of the 3x3 mean over the non-NaN pixels, on the pixels with known == 0 that are
    not NaN (tg_void_smooth); x is left unchanged."""
    H, W = _edt_hw(x, "x")
    _hip(x, torch.float32, (H, W), "x")
    _hip(known, torch.uint8, (H, W), "known")
    steps = int(steps)
    if steps < 0:
        raise L.TgError(f"void_smooth: steps {steps} < 0")
    if steps == 0:
        return x.clone()
    lib = _lib()
    a, b = x, torch.empty_like(x)
    spare = torch.empty_like(x) if steps > 1 else None
    for _ in range(steps):
        L.check(lib.tg_void_smooth(_p(a), _p(known), H, W, _p(b), _stream()), "tg_void_smooth")
        a, b = b, (spare if a is x else a)
    return a


def _ws_make(ws_bytes, name, H, W, device, err=L.TgError):
    """A caller-owned workspace of ws_bytes(H, W) bytes (a tg_*_ws_bytes function); `name` stands in the message."""
    n = ws_bytes(int(H), int(W))
    if n == 0:
        raise err(f"{name}: raster {H}x{W} must be non-empty with H*W < 2^31")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _ws_chk(ws, H, W, ws_bytes, name, who=None, align=1, err=L.TgError):
    """ws is what {name}_ws makes for an H x W raster, or larger; `who` (default: name) stands in the message."""
    need = ws_bytes(H, W)
    if not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= need
            and ws.data_ptr() % align == 0):
        aligned = f", aligned to {align}" if align > 1 else ""
        raise err(f"{who or name}: ws must be a contiguous uint8 HIP tensor of at least {need} bytes{aligned} ({name}_ws)")


DEPFILL_CONNS = (8, 4)


def _depfill_in(z, known, w, conn, who):
    H, W = _raster_hw(z, "z")
    _hip(z, torch.float32, (H, W), "z")
    _hip(known, torch.uint8, (H, W), "known")
    if w is not None:
        _hip(w, torch.float32, (H, W), "w")
        if w.data_ptr() == z.data_ptr():
            raise L.TgError(f"{who}: w must not alias z")
    if conn is not None and (isinstance(conn, bool) or conn not in DEPFILL_CONNS):
        raise L.TgError(f"{who}: connectivity {conn!r} must be 8 or 4")
    return H, W


def depfill_ws(H, W, device):
    """The workspace of one depression fill: uint8 [tg_depfill_ws_bytes]; it carries the dirty tiles from depfill_init through
    the depfill_sweep calls, so it is the caller's and not the shared one."""
    return _ws_make(_lib().tg_depfill_ws_bytes, "depfill", H, W, device)


def depfill_init(z, known, conn, ws):
    """-> w float32 [H][W]: z at the outlets (known pixels on the edge or with an unknown conn-neighbour), +inf at the other
    known pixels, NaN at unknown ones; every tile of ws dirty (tg_depfill_init)."""
    H, W = _depfill_in(z, known, None, conn, "depfill_init")
    _ws_chk(ws, H, W, _lib().tg_depfill_ws_bytes, "depfill")
    w = torch.empty(H, W, dtype=torch.float32, device=z.device)
    L.check(_lib().tg_depfill_init(_p(z), _p(known), H, W, int(conn), _p(w), _p(ws), ws.numel(), _stream()), "tg_depfill_init")
    return w


def depfill_sweep(z, known, conn, n, w, changed, visits, ws):
    """n >= 1 sweeps of w in place; changed int32 [1] = visits of the last sweep that lowered a value (0: a fixed point);
    visits int64 [1] is added to (tg_depfill_sweep)."""
    H, W = _depfill_in(z, known, w, conn, "depfill_sweep")
    _ws_chk(ws, H, W, _lib().tg_depfill_ws_bytes, "depfill")
    _hip(changed, torch.int32, (1,), "changed")
    _hip(visits, torch.int64, (1,), "visits")
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 1 << 20:
        raise L.TgError(f"depfill_sweep: n {n!r} must be an integer in [1, 2^20]")
    L.check(_lib().tg_depfill_sweep(_p(z), _p(known), H, W, int(conn), n, _p(w), _p(changed), _p(visits), _p(ws), ws.numel(),
                                    _stream()), "tg_depfill_sweep")


def depfill_stats(z, w, known, sel=None):
    """-> (counts int64 [3]: pixels with w > z, of those still +inf, pixels counted; sums float64 [2]: the depth sum over the
    raised finite pixels in a fixed order, the largest depth) over the known pixels, with sel (uint8 [H][W]) those with
    sel != 0 (tg_depfill_stats)."""
    H, W = _depfill_in(z, known, w, None, "depfill_stats")
    if sel is not None:
        _hip(sel, torch.uint8, (H, W), "sel")
    counts = torch.empty(3, dtype=torch.int64, device=z.device)
    sums = torch.empty(2, dtype=torch.float64, device=z.device)
    lib = _lib()
    ws = workspace(lib.tg_depfill_ws_bytes(H, W))
    L.check(lib.tg_depfill_stats(_p(z), _p(w), _p(known), _p(sel), H, W, _p(counts), _p(sums), _p(ws), ws.numel() * 4, _stream()),
            "tg_depfill_stats")
    return counts, sums


def depfill_finish(z, w, known, want_depth=False, want_flags=False):
    """-> (out float32 [H][W]: w where raised, z's bits elsewhere, NaN at unknown and unreached pixels; depth float32 or None:
    out - z; flags uint8 or None: 1 where w > z) (tg_depfill_finish)."""
    H, W = _depfill_in(z, known, w, None, "depfill_finish")
    out = torch.empty(H, W, dtype=torch.float32, device=z.device)
    depth = torch.empty(H, W, dtype=torch.float32, device=z.device) if want_depth else None
    flags = torch.empty(H, W, dtype=torch.uint8, device=z.device) if want_flags else None
    L.check(_lib().tg_depfill_finish(_p(z), _p(w), _p(known), H, W, _p(out), _p(depth), _p(flags), _stream()),
            "tg_depfill_finish")
    return out, depth, flags


def flow_ws(H, W, device):
    """The workspace of one flow routing: uint8 [tg_flow_ws_bytes]; it carries the dirty tiles of the flat sweeps and the planes
    of the accumulation from call to call, so it is the caller's and not the shared one."""
    return _ws_make(_lib().tg_flow_ws_bytes, "flow", H, W, device)


def _flow_count(v, lo, hi, name, who):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise L.TgError(f"{who}: {name} {v!r} must be an integer in [{lo}, {hi}]")
    return v


def flow_slope(w, known, ws):
    """-> (dir uint8 [H][W]: 1..8 towards the steepest positive drop, TG_FLOW_OUT, TG_FLOW_UNDECIDED, 0 at unknown pixels;
    D int32 [H][W]: 0 decided, TG_FLOW_FAR undecided, -1 unknown; counts int64 [2]: known pixels, outlets); every tile of ws dirty
    (tg_flow_slope)."""
    H, W = _raster_hw(w, "w")
    _hip(w, torch.float32, (H, W), "w")
    _hip(known, torch.uint8, (H, W), "known")
    _ws_chk(ws, H, W, _lib().tg_flow_ws_bytes, "flow")
    d = torch.empty(H, W, dtype=torch.uint8, device=w.device)
    D = torch.empty(H, W, dtype=torch.int32, device=w.device)
    counts = torch.empty(2, dtype=torch.int64, device=w.device)
    L.check(_lib().tg_flow_slope(_p(w), _p(known), H, W, _p(d), _p(D), _p(counts), _p(ws), ws.numel(), _stream()), "tg_flow_slope")
    return d, D, counts


def flow_flat_sweep(w, n, D, changed, visits, ws):
    """n >= 1 sweeps of D in place; changed int32 [1] = visits of the last sweep that lowered a value (0: a fixed point);
    visits int64 [1] is added to (tg_flow_flat_sweep)."""
    H, W = _raster_hw(w, "w")
    _hip(w, torch.float32, (H, W), "w")
    _hip(D, torch.int32, (H, W), "D")
    _ws_chk(ws, H, W, _lib().tg_flow_ws_bytes, "flow")
    _hip(changed, torch.int32, (1,), "changed")
    _hip(visits, torch.int64, (1,), "visits")
    _flow_count(n, 1, 1 << 20, "n", "flow_flat_sweep")
    L.check(_lib().tg_flow_flat_sweep(_p(w), H, W, n, _p(D), _p(changed), _p(visits), _p(ws), ws.numel(), _stream()),
            "tg_flow_flat_sweep")


def flow_flat_dir(w, D, d):
    """The undecided pixels of d (uint8 [H][W], in place) get their flat code or TG_FLOW_PIT from D -> counts int64 [2]: flat
    pixels, pits (tg_flow_flat_dir)."""
    H, W = _raster_hw(w, "w")
    _hip(w, torch.float32, (H, W), "w")
    _hip(D, torch.int32, (H, W), "D")
    _hip(d, torch.uint8, (H, W), "dir")
    counts = torch.empty(2, dtype=torch.int64, device=w.device)
    L.check(_lib().tg_flow_flat_dir(_p(w), _p(D), H, W, _p(d), _p(counts), _stream()), "tg_flow_flat_dir")
    return counts


def flow_accum_init(d, ws):
    """The pointers and unit sums of the accumulation from the codes d (uint8 [H][W]) into ws (tg_flow_accum_init)."""
    H, W = _raster_hw(d, "dir")
    _hip(d, torch.uint8, (H, W), "dir")
    _ws_chk(ws, H, W, _lib().tg_flow_ws_bytes, "flow")
    L.check(_lib().tg_flow_accum_init(_p(d), H, W, _p(ws), ws.numel(), _stream()), "tg_flow_accum_init")


def flow_accum(H, W, k0, n, state, ws):
    """Rounds k0 .. k0 + n - 1 of the pointer doubling; state int32 [2] = pointers left, rounds that ran (tg_flow_accum)."""
    _ws_chk(ws, int(H), int(W), _lib().tg_flow_ws_bytes, "flow")
    _hip(state, torch.int32, (2,), "state")
    _flow_count(k0, 0, L.TG_FLOW_MAX_ROUNDS, "k0", "flow_accum")
    _flow_count(n, 1, L.TG_FLOW_MAX_ROUNDS - k0, "n", "flow_accum")
    L.check(_lib().tg_flow_accum(int(H), int(W), k0, n, _p(state), _p(ws), ws.numel(), _stream()), "tg_flow_accum")


def flow_accum_finish(H, W, rounds, ws):
    """-> (acc int32 [H][W], amax int32 [1]) after `rounds` rounds (tg_flow_accum_finish)."""
    _ws_chk(ws, int(H), int(W), _lib().tg_flow_ws_bytes, "flow")
    _flow_count(rounds, 0, L.TG_FLOW_MAX_ROUNDS, "rounds", "flow_accum_finish")
    acc = torch.empty(int(H), int(W), dtype=torch.int32, device=ws.device)
    amax = torch.empty(1, dtype=torch.int32, device=ws.device)
    L.check(_lib().tg_flow_accum_finish(int(H), int(W), rounds, _p(acc), _p(amax), _p(ws), ws.numel(), _stream()),
            "tg_flow_accum_finish")
    return acc, amax


FLOW_BASIN_COUNTS, FLOW_COMPARE_COUNTS = L.TG_FLOW_BASIN_COUNTS, L.TG_FLOW_COMPARE_COUNTS
# tg_flow_compare's counters in order
FLOW_COMPARE_NAMES = ("cells", "dir_equal", "dir_routed", "dir_within_45", "same_outlet", "outlet_d2_sum", "outlet_d2_max",
                      "area_octave_sum", "streams_truth", "streams_pred", "streams_both", "pred_matched", "pred_far", "pred_d2_sum",
                      "pred_d2_max", "truth_matched", "truth_far", "truth_d2_sum", "truth_d2_max")


def flow_basin_ws(H, W, device):
    """The workspace of one watershed labelling: uint8 [tg_flow_basin_ws_bytes]; it carries the two planes of records from
    flow_basin_init through the flow_basin calls to flow_basin_finish, so it is the caller's and not the shared one."""
    return _ws_make(_lib().tg_flow_basin_ws_bytes, "flow_basin", H, W, device)


def flow_basin_init(d, pour, ws):
    """The start records of the watershed doubling from the codes d (uint8 [H][W], without TG_FLOW_UNDECIDED) and the pour
    points (uint8 [H][W], nonzero = terminal, or None) into ws -> counts int64 [2]: pour points that became terminals, pour
    points ignored on unknown pixels (tg_flow_basin_init)."""
    H, W = _raster_hw(d, "dir")
    _hip(d, torch.uint8, (H, W), "dir")
    if pour is not None:
        _hip(pour, torch.uint8, (H, W), "pour")
    _ws_chk(ws, H, W, _lib().tg_flow_basin_ws_bytes, "flow_basin", align=16)
    counts = torch.empty(2, dtype=torch.int64, device=d.device)
    L.check(_lib().tg_flow_basin_init(_p(d), _p(pour), H, W, _p(counts), _p(ws), ws.numel(), _stream()), "tg_flow_basin_init")
    return counts


def flow_basin(H, W, k0, n, state, ws):
    """Rounds k0 .. k0 + n - 1 of the watershed doubling; state int32 [2] = pointers left, rounds that ran (tg_flow_basin)."""
    _ws_chk(ws, int(H), int(W), _lib().tg_flow_basin_ws_bytes, "flow_basin", align=16)
    _hip(state, torch.int32, (2,), "state")
    _flow_count(k0, 0, L.TG_FLOW_MAX_ROUNDS, "k0", "flow_basin")
    _flow_count(n, 1, L.TG_FLOW_MAX_ROUNDS - k0, "n", "flow_basin")
    L.check(_lib().tg_flow_basin(int(H), int(W), k0, n, _p(state), _p(ws), ws.numel(), _stream()), "tg_flow_basin")


def flow_basin_finish(H, W, rounds, ws, cellsize=1.0, want_steps=False, want_length=True):
    """-> (basin int32 [H][W]: the last pixel reached, -1 at unknown pixels; nc, nd int32 [H][W] or None: cardinal and diagonal
    steps; length_m float32 [H][W] or None; counts int64 [FLOW_BASIN_COUNTS]: terminals, the largest nc + nd, the bits of the
    largest length) after `rounds` rounds (tg_flow_basin_finish)."""
    H, W = int(H), int(W)
    _ws_chk(ws, H, W, _lib().tg_flow_basin_ws_bytes, "flow_basin", align=16)
    _flow_count(rounds, 0, L.TG_FLOW_MAX_ROUNDS, "rounds", "flow_basin_finish")
    c = float(cellsize)
    if not (c > 0 and c < float("inf")):
        raise L.TgError(f"flow_basin_finish: cellsize {cellsize!r} must be finite and > 0")
    dev = ws.device
    basin = torch.empty(H, W, dtype=torch.int32, device=dev)
    nc = torch.empty(H, W, dtype=torch.int32, device=dev) if want_steps else None
    nd = torch.empty(H, W, dtype=torch.int32, device=dev) if want_steps else None
    length = torch.empty(H, W, dtype=torch.float32, device=dev) if want_length else None
    counts = torch.empty(FLOW_BASIN_COUNTS, dtype=torch.int64, device=dev)
    L.check(_lib().tg_flow_basin_finish(H, W, rounds, c, _p(basin), _p(nc), _p(nd), _p(length), _p(counts), _p(ws), ws.numel(),
                                        _stream()), "tg_flow_basin_finish")
    return basin, nc, nd, length, counts


def flow_compare(sel, dir_t, dir_p, basin_t, basin_p, acc_t, acc_p, d2_t, d2_p, stream_cells, tol2):
    """-> counts int64 [FLOW_COMPARE_COUNTS] (FLOW_COMPARE_NAMES) of two routings over the pixels with sel != 0 and both
    directions != 0 (tg_flow_compare).  sel, dir_*: uint8 [H][W]; basin_*, acc_*, d2_*: int32 [H][W]; sides at most EDT_MAX_SIDE."""
    H, W = _edt_hw(sel, "sel")
    for t, name in ((sel, "sel"), (dir_t, "dir_t"), (dir_p, "dir_p")):
        _hip(t, torch.uint8, (H, W), name)
    for t, name in ((basin_t, "basin_t"), (basin_p, "basin_p"), (acc_t, "acc_t"), (acc_p, "acc_p"), (d2_t, "d2_t"), (d2_p, "d2_p")):
        _hip(t, torch.int32, (H, W), name)
    _flow_count(stream_cells, 1, 2 ** 31 - 1, "stream_cells", "flow_compare")
    _flow_count(tol2, 0, EDT_FAR - 1, "tol2", "flow_compare")
    counts = torch.empty(FLOW_COMPARE_COUNTS, dtype=torch.int64, device=sel.device)
    L.check(_lib().tg_flow_compare(_p(sel), _p(dir_t), _p(dir_p), _p(basin_t), _p(basin_p), _p(acc_t), _p(acc_p), _p(d2_t),
                                   _p(d2_p), H, W, stream_cells, tol2, _p(counts), _stream()), "tg_flow_compare")
    return counts


STREAM_HEAD, STREAM_INTERIOR, STREAM_JUNCTION = L.TG_STREAM_HEAD, L.TG_STREAM_INTERIOR, L.TG_STREAM_JUNCTION
STREAM_ORDER_BINS, STREAM_ORDER_COUNTS = L.TG_STREAM_ORDER_BINS, L.TG_STREAM_ORDER_COUNTS
FLOOD_MAX_STAGES, FLOOD_COUNTS = L.TG_FLOOD_MAX_STAGES, L.TG_FLOOD_COUNTS
# tg_flood_compare's first six counters; then wet_t, wet_p, wet_both for each of the FLOOD_MAX_STAGES stages
FLOOD_NAMES = ("cells", "undrained_t", "undrained_p", "abs_q10", "bias_q10", "abs_max_bits")


def stream_class(d, acc, min_cells, ws):
    """-> (cls uint8 [H][W]: 0, STREAM_HEAD, STREAM_INTERIOR, STREAM_JUNCTION; order int32 [H][W]: 1 on the stream pixels (dir != 0
    and acc >= min_cells), the start of stream_order; counts int64 [4]: stream pixels, heads, junctions, stream terminals); the
    start records of the upstream doubling go into ws (flow_basin_ws) for flow_basin and flow_basin_finish (tg_stream_class)."""
    H, W = _raster_hw(d, "dir")
    _hip(d, torch.uint8, (H, W), "dir")
    _hip(acc, torch.int32, (H, W), "acc")
    _flow_count(min_cells, 1, 2 ** 31 - 1, "min_cells", "stream_class")
    _ws_chk(ws, H, W, _lib().tg_flow_basin_ws_bytes, "flow_basin", align=16)
    cls = torch.empty(H, W, dtype=torch.uint8, device=d.device)
    order = torch.empty(H, W, dtype=torch.int32, device=d.device)
    counts = torch.empty(4, dtype=torch.int64, device=d.device)
    L.check(_lib().tg_stream_class(_p(d), _p(acc), H, W, min_cells, _p(cls), _p(order), _p(counts), _p(ws), ws.numel(), _stream()),
            "tg_stream_class")
    return cls, order, counts


def stream_order(d, cls, top, junctions, n, order, changed):
    """n >= 1 rounds of the Strahler iteration over the junctions (int32 [nj]: the linear indices of the STREAM_JUNCTION pixels),
    order int32 [H][W] in place; changed int32 [1] = raises of the last round (0: a fixed point) (tg_stream_order)."""
    H, W = _raster_hw(d, "dir")
    _hip(d, torch.uint8, (H, W), "dir")
    _hip(cls, torch.uint8, (H, W), "cls")
    _hip(top, torch.int32, (H, W), "top")
    _hip(order, torch.int32, (H, W), "order")
    _hip(changed, torch.int32, (1,), "changed")
    if not (isinstance(junctions, torch.Tensor) and junctions.is_cuda and junctions.dtype == torch.int32 and junctions.dim() == 1
            and junctions.is_contiguous() and junctions.numel() <= H * W):
        raise L.TgError(f"stream_order: junctions must be a contiguous int32 HIP tensor [nj] with nj <= {H * W}")
    _flow_count(n, 1, 1 << 20, "n", "stream_order")
    nj = junctions.numel()
    L.check(_lib().tg_stream_order(_p(d), _p(cls), _p(top), _p(junctions) if nj else None, nj, H, W, n, _p(order), _p(changed),
                                   _stream()), "tg_stream_order")


def stream_order_finish(cls, top, order):
    """-> (out uint8 [H][W]: order[top] on the stream pixels, 0 elsewhere; counts int64 [STREAM_ORDER_COUNTS]: the largest order,
    cells of order 1 .. STREAM_ORDER_BINS, links of order 1 .. STREAM_ORDER_BINS) (tg_stream_order_finish)."""
    H, W = _raster_hw(cls, "cls")
    _hip(cls, torch.uint8, (H, W), "cls")
    _hip(top, torch.int32, (H, W), "top")
    _hip(order, torch.int32, (H, W), "order")
    out = torch.empty(H, W, dtype=torch.uint8, device=cls.device)
    counts = torch.empty(STREAM_ORDER_COUNTS, dtype=torch.int64, device=cls.device)
    L.check(_lib().tg_stream_order_finish(_p(cls), _p(top), _p(order), H, W, _p(out), _p(counts), _stream()),
            "tg_stream_order_finish")
    return out, counts


def hand(w, basin, smask, length_m=None):
    """-> (hand float32 [H][W]: w(p) - w(basin(p)) where the terminal basin(p) is a pixel of smask (uint8 [H][W]), NaN elsewhere;
    distance float32 [H][W] or None: length_m where drained, NaN elsewhere; counts int64 [4]: drained, undrained, drainage
    pixels, the bits of the largest hand) (tg_hand)."""
    H, W = _raster_hw(w, "w")
    _hip(w, torch.float32, (H, W), "w")
    _hip(basin, torch.int32, (H, W), "basin")
    _hip(smask, torch.uint8, (H, W), "stream")
    if length_m is not None:
        _hip(length_m, torch.float32, (H, W), "length_m")
    out = torch.empty(H, W, dtype=torch.float32, device=w.device)
    dist = torch.empty(H, W, dtype=torch.float32, device=w.device) if length_m is not None else None
    counts = torch.empty(4, dtype=torch.int64, device=w.device)
    L.check(_lib().tg_hand(_p(w), _p(basin), _p(smask), _p(length_m), H, W, _p(out), _p(dist), _p(counts), _stream()), "tg_hand")
    return out, dist, counts


def flood_stages(stages):
    """The stages of flood_compare checked on the host: 1 .. FLOOD_MAX_STAGES numbers, each finite and > 0 as float32, strictly
    increasing as float32 -> (L.TgFloodStages, k)."""
    import numpy as np
    try:
        vals = [float(v) for v in stages]
    except (TypeError, ValueError):
        raise L.TgError(f"flood_compare: stages {stages!r} must be a sequence of numbers") from None
    if any(isinstance(v, bool) for v in stages) or not 1 <= len(vals) <= FLOOD_MAX_STAGES:
        raise L.TgError(f"flood_compare: stages {stages!r} must be 1 to {FLOOD_MAX_STAGES} numbers")
    with np.errstate(over="ignore"):
        f = np.array(vals, np.float64).astype(np.float32)
    if not (np.isfinite(f).all() and (f > 0).all()):
        raise L.TgError(f"flood_compare: stages {stages!r} must be finite and > 0 in float32")
    if not (np.diff(f) > 0).all():
        raise L.TgError(f"flood_compare: stages {stages!r} must be strictly increasing in float32")
    st = L.TgFloodStages()
    for i, v in enumerate(f.tolist()):
        st.s[i] = v
    return st, len(vals)


def flood_compare(sel, hand_t, hand_p, stages):
    """-> counts int64 [FLOOD_COUNTS] of two HAND planes (float32 [H][W]) over the pixels with sel != 0 (uint8 [H][W]):
    FLOOD_NAMES, then wet_t, wet_p, wet_both per stage (tg_flood_compare)."""
    H, W = _raster_hw(sel, "sel")
    _hip(sel, torch.uint8, (H, W), "sel")
    _hip(hand_t, torch.float32, (H, W), "hand_t")
    _hip(hand_p, torch.float32, (H, W), "hand_p")
    st, k = flood_stages(stages)
    counts = torch.empty(FLOOD_COUNTS, dtype=torch.int64, device=sel.device)
    L.check(_lib().tg_flood_compare(_p(sel), _p(hand_t), _p(hand_p), H, W, st, k, _p(counts), _stream()), "tg_flood_compare")
    return counts


MFD_MAX_EXPONENT, MFD_COUNTS = L.TG_MFD_MAX_EXPONENT, L.TG_MFD_COUNTS
# tg_mfd_setup's counters in order
MFD_COUNT_NAMES = ("dispersive", "single", "sinks", "not_final", "tile_visits")


def mfd_cdiag(exponent):
    """The weight of a diagonal drop against a cardinal one, 2 ** (-(e + 1) / 2) as a double: Quinn's contour lengths 0.5 and
    sqrt(2) / 4 over the step lengths 1 and sqrt(2).  The kernels and the oracle of the tests get these bits."""
    import numbers
    if isinstance(exponent, bool) or not isinstance(exponent, numbers.Integral) or not 1 <= exponent <= MFD_MAX_EXPONENT:
        raise ValueError(f"mfd: exponent {exponent!r} must be an integer in [1, {MFD_MAX_EXPONENT}]")
    return 2.0 ** (-(int(exponent) + 1) / 2)


def _mfd_plane(t, dtype, shape, name, who):
    """The mfd entries refuse with ValueError, before any launch."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
            and (shape is None or tuple(t.shape) == shape)):
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{who}: {name} must be a contiguous {dtype} HIP tensor {list(shape) if shape else '[H][W]'}, got {got}")


def _mfd_hw(t, name, who):
    _mfd_plane(t, torch.float32, None, name, who)
    if t.dim() != 2 or min(t.shape) < 1 or t.shape[0] * t.shape[1] >= 2 ** 31:
        raise ValueError(f"{who}: {name} must be [H][W], non-empty with H*W < 2^31, got {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[1])


def mfd_ws(H, W, device):
    """The workspace of one MFD accumulation: uint8 [tg_mfd_ws_bytes]; it carries S, the donor bytes and the tile list from
    mfd_setup through the mfd_sweep calls to mfd_finish, so it is the caller's and not the shared one."""
    return _ws_make(_lib().tg_mfd_ws_bytes, "mfd", H, W, device, err=ValueError)


def mfd_setup(w, known, d, exponent, ws):
    """-> (A float64 [H][W]: -1.0 at known pixels (not final), 0.0 at unknown ones; counts int64 [MFD_COUNTS]: MFD_COUNT_NAMES); S,
    the donor bytes and the tile list go into ws (tg_mfd_setup)."""
    who = "mfd_setup"
    cdiag = mfd_cdiag(exponent)
    H, W = _mfd_hw(w, "w", who)
    _mfd_plane(known, torch.uint8, (H, W), "known", who)
    _mfd_plane(d, torch.uint8, (H, W), "dir", who)
    _ws_chk(ws, H, W, _lib().tg_mfd_ws_bytes, "mfd", who=who, align=8, err=ValueError)
    A = torch.empty(H, W, dtype=torch.float64, device=w.device)
    counts = torch.empty(MFD_COUNTS, dtype=torch.int64, device=w.device)
    L.check(_lib().tg_mfd_setup(_p(w), _p(known), _p(d), H, W, int(exponent), cdiag, _p(A), _p(counts), _p(ws), ws.numel(), _stream()),
            "tg_mfd_setup")
    return A, counts


def mfd_sweep(w, exponent, n, A, counts, ws):
    """n >= 1 sweeps of A in place; counts[3] goes down by the pixels made final, counts[4] up by the tiles visited
    (tg_mfd_sweep)."""
    who = "mfd_sweep"
    cdiag = mfd_cdiag(exponent)
    H, W = _mfd_hw(w, "w", who)
    _mfd_plane(A, torch.float64, (H, W), "A", who)
    _mfd_plane(counts, torch.int64, (MFD_COUNTS,), "counts", who)
    _ws_chk(ws, H, W, _lib().tg_mfd_ws_bytes, "mfd", who=who, align=8, err=ValueError)
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 1 << 20:
        raise ValueError(f"{who}: n {n!r} must be an integer in [1, 2^20]")
    L.check(_lib().tg_mfd_sweep(_p(w), H, W, int(exponent), cdiag, n, _p(A), _p(counts), _p(ws), ws.numel(), _stream()), "tg_mfd_sweep")


def mfd_finish(A, d, ws):
    """-> (acc float32 [H][W]: A rounded once; out float64 [2]: the largest A, the sum of A over the sinks in a fixed order)
    (tg_mfd_finish)."""
    who = "mfd_finish"
    _mfd_plane(A, torch.float64, None, "A", who)
    if A.dim() != 2:
        raise ValueError(f"{who}: A must be [H][W], got {tuple(A.shape)}")
    H, W = int(A.shape[0]), int(A.shape[1])
    _mfd_plane(d, torch.uint8, (H, W), "dir", who)
    _ws_chk(ws, H, W, _lib().tg_mfd_ws_bytes, "mfd", who=who, align=8, err=ValueError)
    acc = torch.empty(H, W, dtype=torch.float32, device=A.device)
    out = torch.empty(2, dtype=torch.float64, device=A.device)
    L.check(_lib().tg_mfd_finish(_p(A), _p(d), H, W, _p(acc), _p(out), _p(ws), ws.numel(), _stream()), "tg_mfd_finish")
    return acc, out


def _pos_f32(v, name, who):
    """A finite number > 0 that stays so as float32 -> that float32 as a Python float."""
    import numbers
    import numpy as np
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real):
        raise ValueError(f"{who}: {name} {v!r} must be a number")
    with np.errstate(over="ignore"):
        f = float(np.float32(v))
    if not (f > 0 and f < float("inf")):
        raise ValueError(f"{who}: {name} {v!r} must be finite and > 0 in float32")
    return f


def terrain_slope(w, known, cellsize=1.0):
    """-> slope float32 [H][W]: Horn's tan(beta) of w over the known pixels, NaN at unknown ones (tg_terrain_slope)."""
    who = "terrain_slope"
    H, W = _mfd_hw(w, "w", who)
    _mfd_plane(known, torch.uint8, (H, W), "known", who)
    _pos_f32(cellsize, "cellsize", who)
    den = _pos_f32(8.0 * float(cellsize), "8 * cellsize", who)
    out = torch.empty(H, W, dtype=torch.float32, device=w.device)
    L.check(_lib().tg_terrain_slope(_p(w), _p(known), H, W, den, _p(out), _stream()), "tg_terrain_slope")
    return out


def wetness(acc, slope, known, cellsize=1.0, min_slope=1e-3):
    """-> twi float32 [H][W] = logf(acc * float32(cellsize) / fmaxf(slope, float32(min_slope))), NaN at unknown pixels
    (tg_wetness)."""
    who = "wetness"
    H, W = _mfd_hw(acc, "acc", who)
    _mfd_plane(slope, torch.float32, (H, W), "slope", who)
    _mfd_plane(known, torch.uint8, (H, W), "known", who)
    c = _pos_f32(cellsize, "cellsize", who)
    ms = _pos_f32(min_slope, "min_slope", who)
    out = torch.empty(H, W, dtype=torch.float32, device=acc.device)
    L.check(_lib().tg_wetness(_p(acc), _p(slope), _p(known), H, W, c, ms, _p(out), _stream()), "tg_wetness")
    return out


def wetness_compare(sel, twi_t, twi_p, ws=None):
    """-> (counts int64 [2]: cells, the bits of the largest |d|; sums float64 [3]: of d, |d|, d * d in a fixed order) of
    d = twi_p - twi_t over the pixels with sel != 0 where both are finite (tg_wetness_compare).  ws: an mfd_ws, made here if None."""
    who = "wetness_compare"
    H, W = _mfd_hw(twi_t, "twi_t", who)
    _mfd_plane(twi_p, torch.float32, (H, W), "twi_p", who)
    _mfd_plane(sel, torch.uint8, (H, W), "sel", who)
    if ws is None:
        ws = mfd_ws(H, W, sel.device)
    _ws_chk(ws, H, W, _lib().tg_mfd_ws_bytes, "mfd", who=who, align=8, err=ValueError)
    counts = torch.empty(2, dtype=torch.int64, device=sel.device)
    sums = torch.empty(3, dtype=torch.float64, device=sel.device)
    L.check(_lib().tg_wetness_compare(_p(sel), _p(twi_t), _p(twi_p), H, W, _p(counts), _p(sums), _p(ws), ws.numel(), _stream()),
            "tg_wetness_compare")
    return counts, sums


TEX_OCTAVES, TEX_SCALES, TEX_NSUM = L.TG_TEX_OCTAVES, L.TG_TEX_SCALES, L.TG_TEX_NSUM


def texture_ws(H, W, device=None):
    """The workspace of one texture_compare: uint8 [tg_texture_ws_bytes], one row of partial sums per workgroup; its contents
    do not matter.  device: the current HIP device if None."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return _ws_make(_lib().tg_texture_ws_bytes, "texture", H, W, device, err=ValueError)


def texture_compare(z, p, sel, known, octaves=TEX_OCTAVES, ws=None):
    """-> (counts int64 [TEX_SCALES]: the triples per scale 2 * octave + class; sums float64 [TEX_SCALES][TEX_NSUM]: of d_z d_z,
    d_p d_p and d_z d_p in a fixed order) of the second differences of z and p (float32 [H][W]) at the lags 1, 2, .. 2^(octaves - 1)
    px over the triples centred where sel != 0 whose three pixels are known (both uint8 [H][W]) (tg_texture_compare).  p may be z.
    ws: a texture_ws, made here if None."""
    import numbers
    who = "texture_compare"
    H, W = _mfd_hw(z, "z", who)
    _mfd_plane(p, torch.float32, (H, W), "p", who)
    _mfd_plane(sel, torch.uint8, (H, W), "sel", who)
    _mfd_plane(known, torch.uint8, (H, W), "known", who)
    if isinstance(octaves, bool) or not isinstance(octaves, numbers.Integral) or not 1 <= octaves <= TEX_OCTAVES:
        raise ValueError(f"{who}: octaves {octaves!r} must be an integer in [1, {TEX_OCTAVES}]")
    for t, name in ((p, "p"), (sel, "sel"), (known, "known")):
        if t.device != z.device:
            raise ValueError(f"{who}: {name} is on {t.device}, z on {z.device}")
    if ws is None:
        ws = texture_ws(H, W, z.device)
    _ws_chk(ws, H, W, _lib().tg_texture_ws_bytes, "texture", who=who, align=8, err=ValueError)
    counts = torch.empty(TEX_SCALES, dtype=torch.int64, device=z.device)
    sums = torch.empty(TEX_SCALES, TEX_NSUM, dtype=torch.float64, device=z.device)
    L.check(_lib().tg_texture_compare(_p(z), _p(p), _p(sel), _p(known), H, W, int(octaves), _p(counts), _p(sums), _p(ws),
                                      ws.numel(), _stream()), "tg_texture_compare")
    return counts, sums


VGM_OCTAVES, VGM_SCALES = L.TG_VGM_OCTAVES, L.TG_VGM_SCALES
VGM_MODELS = ("power", "exponential", "spherical")          # TG_VGM_POWER, TG_VGM_EXPONENTIAL, TG_VGM_SPHERICAL


def variogram_ws(H, W, device=None):
    """The workspace of one variogram: uint8 [tg_variogram_ws_bytes], one row of partial sums per workgroup; its contents do
    not matter.  device: the current HIP device if None."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return _ws_make(_lib().tg_variogram_ws_bytes, "variogram", H, W, device, err=ValueError)


def variogram(z, known, octaves=VGM_OCTAVES, ws=None):
    """-> (counts int64 [2 * octaves]: the pairs per scale 2 * octave + class; sums float64 [2 * octaves]: of d * d in a fixed
    order) of the first differences d of z (float32 [H][W]) at the lags 1, 2, .. 2^(octaves - 1) px along the axes (class 0) and
    the diagonals (class 1), over the unordered pairs whose two pixels are known (uint8 [H][W]) (tg_variogram).  The
    semivariance of a scale is sums / (2 counts).  ws: a variogram_ws, made here if None."""
    import numbers
    who = "variogram"
    H, W = _mfd_hw(z, "z", who)
    _mfd_plane(known, torch.uint8, (H, W), "known", who)
    if isinstance(octaves, bool) or not isinstance(octaves, numbers.Integral) or not 1 <= octaves <= VGM_OCTAVES:
        raise ValueError(f"{who}: octaves {octaves!r} must be an integer in [1, {VGM_OCTAVES}]")
    if known.device != z.device:
        raise ValueError(f"{who}: known is on {known.device}, z on {z.device}")
    if ws is None:
        ws = variogram_ws(H, W, z.device)
    _ws_chk(ws, H, W, _lib().tg_variogram_ws_bytes, "variogram", who=who, align=8, err=ValueError)
    counts = torch.empty(VGM_SCALES, dtype=torch.int64, device=z.device)
    sums = torch.empty(VGM_SCALES, dtype=torch.float64, device=z.device)
    L.check(_lib().tg_variogram(_p(z), _p(known), H, W, int(octaves), _p(counts), _p(sums), _p(ws), ws.numel(), _stream()),
            "tg_variogram")
    return counts[:2 * int(octaves)], sums[:2 * int(octaves)]


def krige(z, known, hits, cellsize, model, nugget, scale, shape, d2=None, idx=None):
    """-> (out float32 [H][W], var float32 [H][W] in m^2, counts int64 [3]: by ray samples, by nearest, left NaN): ordinary
    kriging of the pixels with known == 0 from the samples of hits (uint16 [8][H][W], rayfill's with want_hits) under the
    variogram `model` (a name out of VGM_MODELS or its index) with nugget, scale and shape (tg_krige).  d2, idx: edt_nearest's,
    for the pixels without a sample; both or neither."""
    import math
    H, W = _edt_hw(z, "z")
    _hip(z, torch.float32, (H, W), "z")
    _hip(known, torch.uint8, (H, W), "known")
    _hip(hits, torch.uint16, (8, H, W), "hits")
    if isinstance(model, str):
        if model not in VGM_MODELS:
            raise L.TgError(f"krige: model {model!r} must be one of {VGM_MODELS}")
        model = VGM_MODELS.index(model)
    if isinstance(model, bool) or not isinstance(model, int) or not 0 <= model < len(VGM_MODELS):
        raise L.TgError(f"krige: model {model!r} must be one of {VGM_MODELS} or its index")
    c, nugget, scale, shape = float(cellsize), float(nugget), float(scale), float(shape)
    if not (math.isfinite(c) and c > 0):
        raise L.TgError(f"krige: cellsize {cellsize!r} must be finite and > 0")
    if not (math.isfinite(nugget) and nugget >= 0):
        raise L.TgError(f"krige: nugget {nugget!r} must be finite and >= 0")
    if not (math.isfinite(scale) and scale > 0):
        raise L.TgError(f"krige: scale {scale!r} must be finite and > 0")
    if not (math.isfinite(shape) and shape > 0 and (model != 0 or shape < 2)):
        raise L.TgError(f"krige: shape {shape!r} must lie in (0, 2) for the power model, else be finite and > 0")
    if (d2 is None) != (idx is None):
        raise L.TgError("krige: d2 and idx go together")
    if d2 is not None:
        _hip(d2, torch.int32, (H, W), "d2")
        _hip(idx, torch.int32, (H, W), "idx")
    out = torch.empty(H, W, dtype=torch.float32, device=z.device)
    var = torch.empty(H, W, dtype=torch.float32, device=z.device)
    counts = torch.empty(3, dtype=torch.int64, device=z.device)
    L.check(_lib().tg_krige(_p(z), _p(known), _p(hits), H, W, c, model, nugget, scale, shape, _p(d2), _p(idx), _p(out),
                            _p(var), _p(counts), _stream()), "tg_krige")
    return out, var, counts


SIM_MAX_WAVES = L.TG_SIM_MAX_WAVES


def sim_field(H, W, waves, origin=(0, 0), nugget_amp=0.0, seed=0, realisation=0):
    """-> u float32 [H][W]: the unconditional random field sum_k amp_k cos(2 pi (fx_k X + fy_k Y + phase_k) / 2^32) + nugget_amp
    * g at the global pixels (Y, X) = origin + (y, x) (tg_sim_field).  waves: a HIP int32 tensor [n][4], n in 1 .. SIM_MAX_WAVES,
    of (fx, fy, phase, the bits of the float32 amp); g: the unit-variance hash noise of (seed, realisation, X, Y)."""
    import math
    import numbers
    who = "sim_field"
    for name, v in (("H", H), ("W", W)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 1 <= v <= EDT_MAX_SIDE:
            raise ValueError(f"{who}: {name} {v!r} must be an integer in [1, {EDT_MAX_SIDE}]")
    if not (isinstance(waves, torch.Tensor) and waves.is_cuda and waves.dtype == torch.int32 and waves.is_contiguous()
            and waves.dim() == 2 and waves.shape[1] == 4 and 1 <= waves.shape[0] <= SIM_MAX_WAVES):
        got = f"{waves.dtype} {tuple(waves.shape)} on {waves.device}" if isinstance(waves, torch.Tensor) else type(waves).__name__
        raise ValueError(f"{who}: waves must be a contiguous int32 HIP tensor [n][4], n in [1, {SIM_MAX_WAVES}], got {got}")
    try:
        y0, x0 = origin
    except (TypeError, ValueError):
        raise ValueError(f"{who}: origin {origin!r} must be (row, column)") from None
    for name, v in (("origin row", y0), ("origin column", x0), ("seed", seed), ("realisation", realisation)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v < 2 ** 32:
            raise ValueError(f"{who}: {name} {v!r} must be an integer in [0, 2^32)")
    a = float(nugget_amp)
    if not (math.isfinite(a) and a >= 0):
        raise ValueError(f"{who}: nugget_amp {nugget_amp!r} must be finite and >= 0")
    u = torch.empty(int(H), int(W), dtype=torch.float32, device=waves.device)
    L.check(_lib().tg_sim_field(_p(u), int(H), int(W), int(x0), int(y0), _p(waves), int(waves.shape[0]), a, int(seed),
                                int(realisation), _stream()), "tg_sim_field")
    return u


def sim_combine(z, known, zk, u, uk, s1=None, s2=None):
    """-> out float32 [H][W]: z bit for bit on known pixels, zk + (u - uk) on the others (tg_sim_combine).  s1, s2: float64
    [H][W] running sums (both or neither), to which an unknown pixel adds u - uk and its square, in place."""
    who = "sim_combine"
    H, W = _mfd_hw(z, "z", who)
    _mfd_plane(known, torch.uint8, (H, W), "known", who)
    for name, t in (("zk", zk), ("u", u), ("uk", uk)):
        _mfd_plane(t, torch.float32, (H, W), name, who)
    if (s1 is None) != (s2 is None):
        raise ValueError(f"{who}: s1 and s2 go together")
    if s1 is not None:
        _mfd_plane(s1, torch.float64, (H, W), "s1", who)
        _mfd_plane(s2, torch.float64, (H, W), "s2", who)
        if s1.data_ptr() == s2.data_ptr():
            raise ValueError(f"{who}: s1 and s2 must be distinct")
    out = torch.empty(H, W, dtype=torch.float32, device=z.device)
    L.check(_lib().tg_sim_combine(_p(out), _p(z), _p(known), _p(zk), _p(u), _p(uk), _p(s1), _p(s2), H, W, _stream()),
            "tg_sim_combine")
    return out


def sim_stats(zk, s1, s2, n):
    """-> (mean float32 [H][W] = zk + s1 / n, sd float32 [H][W] = sqrt(max(0, (s2 - s1^2 / n) / (n - 1)))) of n >= 2
    realisations from sim_combine's running sums; sd is 0 on known pixels and NaN where zk is (tg_sim_stats)."""
    import numbers
    who = "sim_stats"
    H, W = _mfd_hw(zk, "zk", who)
    _mfd_plane(s1, torch.float64, (H, W), "s1", who)
    _mfd_plane(s2, torch.float64, (H, W), "s2", who)
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 2 <= n < 2 ** 31:
        raise ValueError(f"{who}: n {n!r} must be an integer >= 2")
    mean = torch.empty(H, W, dtype=torch.float32, device=zk.device)
    sd = torch.empty(H, W, dtype=torch.float32, device=zk.device)
    L.check(_lib().tg_sim_stats(_p(mean), _p(sd), _p(zk), _p(s1), _p(s2), int(n), H, W, _stream()), "tg_sim_stats")
    return mean, sd


VFILL_NSTATS = 4                                # tg_vfill_setup stats: known, unknown, min bits, max bits


def vfill_ws(H, W, device):
    """A workspace for one fill of an H x W raster (tg_vfill_ws_bytes; 256-byte aligned by the caching allocator)."""
    nb = _lib().tg_vfill_ws_bytes(int(H), int(W))
    if nb == 0:
        raise L.TgError(f"vfill: raster {H}x{W} must be non-empty with H*W < 2^31")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def vfill_setup(dem, mask, nodata, ws):
    """-> stats int64 [VFILL_NSTATS] (tg_vfill_setup): known map, statistics, initial guess, level flags and tile lists."""
    H, W = _raster_hw(dem, "dem")
    _hip(dem, torch.float32, (H, W), "dem")
    if mask is not None:
        _hip(mask, torch.float32, (H, W), "mask")
    _hip(ws, torch.uint8, (ws.numel(),), "ws")
    stats = torch.empty(VFILL_NSTATS, dtype=torch.int64, device=dem.device)
    L.check(_lib().tg_vfill_setup(_p(dem), _p(mask), int(nodata is not None), 0.0 if nodata is None else float(nodata), H, W,
                                  _p(ws), ws.numel(), _p(stats), _stream()), "tg_vfill_setup")
    return stats


def vfill_cycle(H, W, ws, change):
    """One V-cycle (tg_vfill_cycle); change int32 [1] gets the float bits of the largest change over the unknowns."""
    _hip(ws, torch.uint8, (ws.numel(),), "ws")
    _hip(change, torch.int32, (1,), "change")
    L.check(_lib().tg_vfill_cycle(int(H), int(W), _p(ws), ws.numel(), _p(change), _stream()), "tg_vfill_cycle")


def vfill_finish(dem, ws, out=None):
    """-> out float32 [H][W]: dem at the known pixels, the solution at the unknowns (tg_vfill_finish)."""
    H, W = _raster_hw(dem, "dem")
    _hip(dem, torch.float32, (H, W), "dem")
    _hip(ws, torch.uint8, (ws.numel(),), "ws")
    out = torch.empty(H, W, dtype=torch.float32, device=dem.device) if out is None else out
    _hip(out, torch.float32, (H, W), "out")
    L.check(_lib().tg_vfill_finish(_p(dem), H, W, _p(ws), ws.numel(), _p(out), _stream()), "tg_vfill_finish")
    return out


def vfill_pcg_ws(H, W, device):
    """The second workspace of the pcg solver (tg_vfill_pcg_ws_bytes): r, z, p twice, the down-pass scratch, partials, scalars."""
    nb = _lib().tg_vfill_pcg_ws_bytes(int(H), int(W))
    if nb == 0:
        raise L.TgError(f"vfill: raster {H}x{W} must be non-empty with H*W < 2^31")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def vfill_pcg_start(H, W, ws, pws):
    """After vfill_setup: the residual, z = M r, the first direction and its step length (tg_vfill_pcg_start)."""
    _hip(ws, torch.uint8, (ws.numel(),), "ws")
    _hip(pws, torch.uint8, (pws.numel(),), "pws")
    L.check(_lib().tg_vfill_pcg_start(int(H), int(W), _p(ws), ws.numel(), _p(pws), pws.numel(), _stream()), "tg_vfill_pcg_start")


def vfill_pcg_iter(H, W, ws, pws, state):
    """One iteration = one V-cycle (tg_vfill_pcg_iter); state int32 [2] gets the float bits of the largest change over the
    unknowns and the number of restarted directions."""
    _hip(ws, torch.uint8, (ws.numel(),), "ws")
    _hip(pws, torch.uint8, (pws.numel(),), "pws")
    _hip(state, torch.int32, (2,), "state")
    L.check(_lib().tg_vfill_pcg_iter(int(H), int(W), _p(ws), ws.numel(), _p(pws), pws.numel(), _p(state), _p(state[1:]),
                                     _stream()), "tg_vfill_pcg_iter")


def vfill_bih_ws(H, W, device):
    """The workspace of the biharmonic fill (tg_vfill_bih_ws_bytes): x twice and the residual in fp64, the fp32 vectors of the
    outer loop and of the inner solve, partials, scalars."""
    nb = _lib().tg_vfill_bih_ws_bytes(int(H), int(W))
    if nb == 0:
        raise L.TgError(f"vfill: raster {H}x{W} must be non-empty with H*W < 2^31")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def vfill_bih_start(H, W, ws, bws, inner):
    """After vfill_setup: the residual, z = G(G(r)), the first direction and its step length (tg_vfill_bih_start)."""
    _hip(ws, torch.uint8, (ws.numel(),), "ws")
    _hip(bws, torch.uint8, (bws.numel(),), "bws")
    L.check(_lib().tg_vfill_bih_start(int(H), int(W), _p(ws), ws.numel(), _p(bws), bws.numel(), int(inner), _stream()),
            "tg_vfill_bih_start")


def vfill_bih_iter(H, W, ws, bws, inner, state):
    """One outer iteration = 2 * inner V-cycles (tg_vfill_bih_iter); state int32 [2] gets the float bits of the largest change
    over the unknowns and the number of restarted directions."""
    _hip(ws, torch.uint8, (ws.numel(),), "ws")
    _hip(bws, torch.uint8, (bws.numel(),), "bws")
    _hip(state, torch.int32, (2,), "state")
    L.check(_lib().tg_vfill_bih_iter(int(H), int(W), _p(ws), ws.numel(), _p(bws), bws.numel(), int(inner), _p(state),
                                     _p(state[1:]), _stream()), "tg_vfill_bih_iter")


SEAM_NCOUNTS = 4                                  # tg_seam_delta counts: ring, interior, unfilled, max |delta| bits


def _seam_in(dem, mask, filled, order=None):
    H, W = _raster_hw(dem, "dem")
    _hip(dem, torch.float32, (H, W), "dem")
    if mask is not None:
        _hip(mask, torch.float32, (H, W), "mask")
    _hip(filled, torch.float32, (H, W), "filled")
    if order is not None and (isinstance(order, bool) or order not in (0, 1)):
        raise L.TgError(f"seam: order {order!r} must be 0 or 1")
    return H, W


def seam_delta(dem, mask, nodata, filled, order=1):
    """-> (delta float32 [H][W], counts int32 [SEAM_NCOUNTS] device) (tg_seam_delta): the ring targets minus the fill, 0 at the
    known pixels and the unfilled holes, NaN at the filled holes without a known 4-neighbour."""
    H, W = _seam_in(dem, mask, filled, order)
    delta = torch.empty(H, W, dtype=torch.float32, device=dem.device)
    counts = torch.empty(SEAM_NCOUNTS, dtype=torch.int32, device=dem.device)
    L.check(_lib().tg_seam_delta(_p(dem), _p(mask), int(nodata is not None), 0.0 if nodata is None else float(nodata),
                                 _p(filled), H, W, int(order), _p(delta), _p(counts), _stream()), "tg_seam_delta")
    return delta, counts


def seam_apply(dem, mask, nodata, filled, delta_filled):
    """-> out float32 [H][W]: dem at the known pixels, filled + delta_filled at the filled holes, NaN at the unfilled ones
    (tg_seam_apply)."""
    H, W = _seam_in(dem, mask, filled)
    _hip(delta_filled, torch.float32, (H, W), "delta_filled")
    out = torch.empty(H, W, dtype=torch.float32, device=dem.device)
    L.check(_lib().tg_seam_apply(_p(dem), _p(mask), int(nodata is not None), 0.0 if nodata is None else float(nodata),
                                 _p(filled), _p(delta_filled), H, W, _p(out), _stream()), "tg_seam_apply")
    return out


def _resample(fn, name, dem, mask, nodata, p, q, keep, extra, out_shape, count_only=False):
    H, W = _raster_hw(dem, "dem")
    _hip(dem, torch.float32, (H, W), "dem")
    if mask is not None:
        _hip(mask, torch.float32, (H, W), "mask")
    p, q = int(p), int(q)
    if p < 1 or q < 1:
        raise L.TgError(f"{name}: scale {p}/{q} must be positive")
    Ho, Wo = -(-H * q // p), -(-W * q // p)
    if out_shape is not None:
        if not (1 <= out_shape[0] <= Ho and 1 <= out_shape[1] <= Wo):
            raise L.TgError(f"{name}: output {tuple(out_shape)} is no top-left crop of the {Ho}x{Wo} grid of scale {p}/{q}")
        Ho, Wo = int(out_shape[0]), int(out_shape[1])
    kd, km, knd = (None, None, None) if keep is None else keep
    for t, nm in ((kd, "keep_dem"), (km, "keep_mask")):
        if t is not None:
            _hip(t, torch.float32, (Ho, Wo), nm)
    out = None if count_only else torch.empty(Ho, Wo, dtype=torch.float32, device=dem.device)
    omask = None if count_only else torch.empty(Ho, Wo, dtype=torch.float32, device=dem.device)
    n_nan = torch.empty(1, dtype=torch.int32, device=dem.device)
    L.check(fn(_p(dem), _p(mask), int(nodata is not None), 0.0 if nodata is None else float(nodata), H, W, p, q, *extra,
               _p(kd), _p(km), int(knd is not None), 0.0 if knd is None else float(knd), Ho, Wo, _p(out), _p(omask), _p(n_nan),
               _stream()), name)
    return out, omask, n_nan


def resample_area(dem, mask, nodata, p, q, cov_num=1, cov_den=2, keep=None, out_shape=None, count_only=False):
    """To the coarser grid of scale p / q >= 1 (tg_resample_area) -> (out float32 [Ho][Wo] with NaN at the unknown pixels,
    known mask float32 1 / 0, n_nan int32 [1] device counter).  An output pixel is known iff its known coverage is positive and
    at least cov_num / cov_den of its clipped footprint.  keep: None or (dem, mask or None, nodata or None) on the output
    grid, whose known pixels are copied through bit for bit.  out_shape: a top-left crop of the output grid (the return trip
    to a native grid).  count_only: write no raster, return (None, None, n_nan)."""
    return _resample(_lib().tg_resample_area, "tg_resample_area", dem, mask, nodata, p, q, keep, (int(cov_num), int(cov_den)),
                     out_shape, count_only)


def raster_count_unknown(dem, mask, nodata):
    """-> int32 [1] device counter: the unknown pixels of (dem, mask, nodata).  tg_resample_area at scale 1 with no output:
    the raster is read once and nothing is written."""
    return resample_area(dem, mask, nodata, 1, 1, count_only=True)[2]


def resample_interp(dem, mask, nodata, p, q, keep=None, out_shape=None):
    """To the finer grid of scale p / q <= 1 (tg_resample_interp): bicubic where all 16 taps are known, else bilinear over the
    known ones of the 4 nearest; returns as resample_area does."""
    return _resample(_lib().tg_resample_interp, "tg_resample_interp", dem, mask, nodata, p, q, keep, (), out_shape)


def _dense_layouts(t):
    """Which dense physical orders a tensor's strides describe: 'c' (row-major) and/or 'cl'."""
    out = set()
    if t.is_contiguous():
        out.add("c")
    if t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous():
        out.add("cl")
    return out


def adam_(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """In-place Adam on the physical storage of p/g/m/v (which must share one dense layout)."""
    lay = _dense_layouts(p)
    for t, nm in ((g, "g"), (m, "m"), (v, "v")):
        if t.shape != p.shape or not (_dense_layouts(t) & lay):
            raise L.TgError(f"adam_: {nm} layout {tuple(t.shape)}/{t.stride()} differs from the parameter's "
                            f"{tuple(p.shape)}/{p.stride()}")
    L.check(_lib().tg_adam(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, step, grad_scale, _stream()), "tg_adam")
    weights_updated([p])


ADAM_CHUNK = 1 << 14
_adam_tables = {}
adam_scalar_arena = None      # set by tg_hip.graph while a train step is captured / replayed: see AdamScalarArena


class AdamLaunch:
    """What one captured adam_multi_ launch has baked in beside its slot's (lr, beta1, beta2, step): eps and grad_scale (kernel
    arguments), the pointers in its device table (which it keeps alive: _adam_tables may be cleared) and its owner -- None, or
    (torch optimiser, index of the param_group, its Parameters in the launch's order), through which the live values are read."""

    def __init__(self, lr, eps, grad_scale, params, ms, vs, owner, refs):
        self.lr, self.eps, self.grad_scale = lr, eps, grad_scale
        self.ptrs = [t.data_ptr() for pmv in zip(params, ms, vs) for t in pmv]
        self.owner, self.refs = owner, refs

    def live_lr(self):
        if self.owner is None:
            return self.lr
        return float(self.owner[0].param_groups[self.owner[1]]["lr"])

    def live_ptrs(self):
        """Parameter and moment pointers as hip_adam_step would find them now (None: a state entry is gone)."""
        if self.owner is None:
            return self.ptrs
        state, out = self.owner[0].state, []
        for p in self.owner[2]:
            st = state.get(p)
            if not st:
                return None
            out += (p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())
        return out


class AdamScalarArena:
    """Per-step Adam scalars in device memory (tg_adam_multi_s) for hipGraph replay.  While `active` (during capture),
    every adam_multi_ call takes the next slot and remembers (lr, betas, step) and its AdamLaunch.  `refresh(k)` recomputes
    every slot for `k` steps later on the host (tg_adam_scalars: the very two floats the eager launch would have been given)
    and writes them to the device through kernel arguments (tg_write_floats, <= 8 slots per launch) on the current stream.
    The learning rate is read from the slot's live param_group at every refresh; the betas, eps and grad_scale are kernel
    arguments of the captured launch and the pointers sit in its device table: `launches` keeps them for the owner of the
    graph to hold against the live optimiser (tg_hip.graph)."""

    def __init__(self, device, nslots=8):
        import numpy as np
        self.dev = torch.zeros(nslots, 2, dtype=torch.float32, device=device)
        self.host = np.zeros((nslots, 2), dtype=np.float32)
        self.slots, self.launches, self.active = [], [], False

    def take(self, lr, beta1, beta2, step, launch=None):
        i = len(self.slots)
        if i >= self.dev.shape[0]:
            raise L.TgError("AdamScalarArena: more optimiser launches per step than slots")
        self.slots.append((lr, beta1, beta2, int(step)))
        self.launches.append(launch)
        return self.dev[i]

    def refresh(self, k):
        lib = _lib()
        for i, ((lr, b1, b2, step), launch) in enumerate(zip(self.slots, self.launches)):
            if launch is not None:
                lr = launch.live_lr()
            L.check(lib.tg_adam_scalars(lr, b1, b2, step + k, C.c_void_p(self.host[i].ctypes.data)), "tg_adam_scalars")
        n = 2 * len(self.slots)
        if n:
            L.check(lib.tg_write_floats(_p(self.dev), n, C.c_void_p(self.host.ctypes.data), _stream()), "tg_write_floats")


def adam_table_key(params, grads, ms, vs):
    """Everything the cached device table of adam_multi_ is built from: the four pointers AND the element count of every
    segment (equal pointers with other counts -- views into one buffer, a pointer the allocator handed out again -- are
    another table)."""
    return (tuple(t.data_ptr() for ts in (params, grads, ms, vs) for t in ts), tuple(p.numel() for p in params))


def adam_multi_(params, grads, ms, vs, lr, beta1, beta2, eps, step, grad_scale=1.0, owner=None):
    """One-launch Adam over many tensors.  The (p, g, m, v, n) table and the work list live on the device and are
    rebuilt only when a pointer changes (persistent gradient buffers keep them stable step after step).
    owner: see AdamLaunch (used while a step is captured only)."""
    import numpy as np
    key = adam_table_key(params, grads, ms, vs)
    ent = _adam_tables.get(key)
    if ent is None:
        lay = None
        for p, g, m, v in zip(params, grads, ms, vs):
            lay = _dense_layouts(p)
            for t, nm in ((g, "g"), (m, "m"), (v, "v")):
                if t.shape != p.shape or not (_dense_layouts(t) & lay):
                    raise L.TgError(f"adam_multi_: {nm} layout differs from the parameter's ({tuple(p.shape)}/{p.stride()})")
        seg = np.zeros((len(params), 5), dtype=np.int64)
        work = []
        for i, (p, g, m, v) in enumerate(zip(params, grads, ms, vs)):
            seg[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
            work += [(i, c) for c in range((p.numel() + ADAM_CHUNK - 1) // ADAM_CHUNK)]
        dev = params[0].device
        ent = (torch.from_numpy(seg).to(dev), torch.tensor(work, dtype=torch.int32).to(dev), len(work))
        if len(_adam_tables) > 64:
            _adam_tables.clear()
        _adam_tables[key] = ent
    segs, work, nwork = ent
    if adam_scalar_arena is not None and adam_scalar_arena.active:
        scal = adam_scalar_arena.take(lr, beta1, beta2, step, AdamLaunch(lr, eps, grad_scale, params, ms, vs, owner, (segs, work)))
        L.check(_lib().tg_adam_multi_s(C.c_void_p(segs.data_ptr()), C.c_void_p(work.data_ptr()), nwork, ADAM_CHUNK, beta1, beta2,
                                       eps, _p(scal), grad_scale, _stream()), "tg_adam_multi_s")
    else:
        L.check(_lib().tg_adam_multi(C.c_void_p(segs.data_ptr()), C.c_void_p(work.data_ptr()), nwork, ADAM_CHUNK, lr, beta1, beta2,
                                     eps, step, grad_scale, _stream()), "tg_adam_multi")
    weights_updated(params)          # prepared conv weights of these tensors are stale now


def axpby_(x, a, b, y):
    """y = a*x + b*y (same dense layout)."""
    assert x.shape == y.shape and (_dense_layouts(x) & _dense_layouts(y)), (x.shape, x.stride(), y.stride())
    L.check(_lib().tg_axpby(_p(x), a, b, _p(y), y.numel(), _stream()), "tg_axpby")
    return y


def lincomb(x, a, y, b):
    _chk(x, "x"); _chk(y, "y")
    _same_numel(x, "x", y=y)
    out = torch.empty_like(x)
    L.check(_lib().tg_lincomb(_p(x), a, _p(y), b, _p(out), x.numel(), _stream()), "tg_lincomb")
    return out


def mul(a, b, keep=None):
    """a*b; keep (optional, same shape, contiguous): also receives a copy of `a` from the same pass (tg_mul_keep)."""
    _chk(a, "a"); _chk(b, "b"); _chk(keep, "keep")
    out = torch.empty_like(a)
    if keep is not None:
        assert keep.numel() == a.numel()
        L.check(_lib().tg_mul_keep(_p(a), _p(b), _p(out), _p(keep), a.numel(), _stream()), "tg_mul_keep")
    else:
        L.check(_lib().tg_mul(_p(a), _p(b), _p(out), a.numel(), _stream()), "tg_mul")
    return out


def nchw_to_nhwc(x):
    """Logical [B,C,H,W] contiguous tensor -> [B,H,W,C] contiguous (C==1 is a free reshape)."""
    B, Cc, H, W = x.shape
    x = x if x.is_contiguous() else x.contiguous()
    if Cc == 1:
        return x.reshape(B, H, W, 1)
    y = empty(B, H, W, Cc, like=x)
    L.check(_lib().tg_nchw_to_nhwc(_p(x), B, Cc, H, W, _p(y), _stream()), "tg_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x):
    B, H, W, Cc = x.shape
    if Cc == 1:
        return x.reshape(B, 1, H, W)
    y = empty(B, Cc, H, W, like=x)
    L.check(_lib().tg_nhwc_to_nchw(_p(x), B, Cc, H, W, _p(y), _stream()), "tg_nhwc_to_nchw")
    return y
