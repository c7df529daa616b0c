"""numpy fp64 oracle of the pointwise kernels (csrc/pointwise.hip: pixel losses, L1 and BCE means, the sigmoid/composite head,
Adam, BN eval statistics, act_bwd) and the error measure the GPU tests judge them by.  Plain restatements of the formulas,
independent of the package: nothing here imports tg_hip, torch or the oracle/ package.  Inputs are converted to float64 on
entry, so a test evaluates the oracle on the very fp32 values the kernel reads."""
import numpy as np

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


# ---- the error measure ------------------------------------------------------------------------------------------------------
def err(x, ref, floor=1e-3):
    """e(x) = max_i |x_i - ref_i| / (|ref_i| + s), s = floor * max|ref|: per element, so a small entry cannot hide behind a
    large one by more than 1/floor.  An all-zero reference is compared absolutely (s = 1); NaN/Inf in x give inf."""
    x, ref = f64(x), f64(ref)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if x.size == 0:
        return 0.0
    if not np.isfinite(x).all():
        return float("inf")
    s = floor * float(np.abs(ref).max())
    if s == 0.0:
        s = 1.0
    return float((np.abs(x - ref) / (np.abs(ref) + s)).max())


# ---- pixel losses --------------------------------------------------------------------------------------------------------
def _window_max(a):
    """3x3 maximum over the taps that lie inside the image (max_pool2d(a, 3, 1, 1): its padding never wins)."""
    B, H, W = a.shape
    p = np.full((B, H + 2, W + 2), -np.inf)
    p[:, 1:-1, 1:-1] = a
    out = np.full((B, H, W), -np.inf)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, p[:, dy:dy + H, dx:dx + W])
    return out


def band(mask):
    """3x3 morphological gradient of the mask: clamp(dilate(m) - erode(m), 0, 1), erode(m) = 1 - dilate(1 - m)."""
    m = f64(mask)
    return np.clip(_window_max(m) - (1.0 - _window_max(1.0 - m)), 0.0, 1.0)


def pixel_losses(pred, target, mask, w_l1, w_tv, w_bnd, l1_weight=None, gscale=None, dpred0=None, eps=1e-6):
    """-> (dict l1, tv, boundary, band_sum, total; dpred [B][H][W]).
    l1 = mean(|p - t| * l1_weight); tv = 2 (sum dh^2 / count_h + sum dw^2 / count_w) / B over xh = p (1 - m) (count_* already
    holds B: the reference divides by the batch twice); boundary = sum(|p - t| band) / (sum(band) + eps), and 0 -- value and
    gradient -- when sum(band) < 1 or the quotient is not finite; total = w_l1 l1 + w_tv tv + w_bnd boundary.
    dpred = gscale * d total / d pred (gscale None = 1), added to dpred0 when that is given."""
    p, t, m, lw, d0 = f64(pred), f64(target), f64(mask), f64(l1_weight), f64(dpred0)
    B, H, W = p.shape
    n = float(B * H * W)
    diff = p - t
    ad = np.abs(diff)
    lwv = np.ones_like(p) if lw is None else lw
    l1 = float((ad * lwv).sum() / n)
    hole = 1.0 - m
    xh = p * hole
    dh = xh[:, 1:, :] - xh[:, :-1, :]
    dw = xh[:, :, 1:] - xh[:, :, :-1]
    count_h, count_w = float(B * (H - 1) * W), float(B * H * (W - 1))
    tv = float(2.0 * ((dh * dh).sum() / count_h + (dw * dw).sum() / count_w) / B)
    bd = band(m)
    den = float(bd.sum())
    on = den >= 1.0
    bnd = 0.0
    if on:
        bnd = float((ad * bd).sum() / (den + eps))
        if not np.isfinite(bnd):
            bnd, on = 0.0, False
    total = w_l1 * l1 + w_tv * tv + w_bnd * bnd
    gs = 1.0 if gscale is None else float(np.asarray(gscale, dtype=np.float64).reshape(-1)[0])
    sg = np.sign(diff)
    g = (w_l1 / n) * sg * lwv
    gx = np.zeros_like(p)                            # d tv / d xh
    ch, cw = 4.0 / (B * count_h), 4.0 / (B * count_w)
    gx[:, 1:, :] += ch * dh
    gx[:, :-1, :] -= ch * dh
    gx[:, :, 1:] += cw * dw
    gx[:, :, :-1] -= cw * dw
    g = g + w_tv * hole * gx
    if on:
        g = g + (w_bnd / (den + eps)) * sg * bd
    g = gs * g
    if d0 is not None:
        g = d0 + g
    return {"l1": l1, "tv": tv, "boundary": bnd, "band_sum": den, "total": total}, g


OUT5 = ("l1", "tv", "boundary", "band_sum", "total")


# ---- L1 mean, BCE with logits -------------------------------------------------------------------------------------------
def l1_mean(a, b, coef=1.0, gscale=None, relu_gate=False):
    """-> (mean |a - b|, da = coef * gscale / n * sign(a - b), and 0 where the gate a > 0 is closed)."""
    a, b = f64(a), f64(b)
    gs = 1.0 if gscale is None else float(np.asarray(gscale, dtype=np.float64).reshape(-1)[0])
    d = a - b
    da = (coef * gs / a.size) * np.sign(d)
    if relu_gate:
        da = np.where(a > 0, da, 0.0)
    return float(np.abs(d).mean()), da


def sigmoid(z):
    """Finite for every z: exp is only ever taken of -|z|."""
    z = f64(z)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_logits(z, target, coef=1.0, gscale=None):
    """Mean binary cross-entropy of sigmoid(z) against the constant `target`, in the form that stays finite at |z| = 90:
    max(z, 0) - z t + log1p(exp(-|z|)); dz = coef * gscale / n * (sigmoid(z) - t)."""
    z = f64(z)
    gs = 1.0 if gscale is None else float(np.asarray(gscale, dtype=np.float64).reshape(-1)[0])
    loss = np.maximum(z, 0.0) - z * target + np.log1p(np.exp(-np.abs(z)))
    return float(loss.mean()), (coef * gs / z.size) * (sigmoid(z) - target)


# ---- generator head ---------------------------------------------------------------------------------------------------------
def sigmoid_composite_fwd(logits, x, mask):
    z, x, m = f64(logits), f64(x), f64(mask)
    return sigmoid(z) * (1.0 - m) + x * m


def sigmoid_composite_bwd(dout, logits, mask):
    """-> (dlogits, dx)."""
    g, z, m = f64(dout), f64(logits), f64(mask)
    return g * (1.0 - m) * sigmoid(z) * sigmoid(-z), g * m


# ---- Adam ------------------------------------------------------------------------------------------------------------------
def adam_scalars(lr, beta1, beta2, step):
    """The two per-step scalars: step_size = lr / (1 - beta1^step), sqrt(1 - beta2^step)."""
    return lr / (1.0 - beta1 ** step), (1.0 - beta2 ** step) ** 0.5


def adam(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) on g * grad_scale, `step` 1-based -> new (p, m, v)."""
    p, g, m, v = f64(p), f64(g) * grad_scale, f64(m), f64(v)
    m = m + (1.0 - beta1) * (g - m)                               # exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g                         # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    step_size, bc2_sqrt = adam_scalars(lr, beta1, beta2, step)
    denom = np.sqrt(v) / bc2_sqrt + eps                           # (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    return p - step_size * (m / denom), m, v                      # param.addcdiv_(exp_avg, denom, value=-step_size)


# ---- small helpers ----------------------------------------------------------------------------------------------------------
def bn_eval_stats(running_mean, running_var, eps=1e-5):
    return f64(running_mean).copy(), 1.0 / np.sqrt(f64(running_var) + eps)


def act_bwd(dout, out, act, slope=0.0, ratio=None):
    """din[r][c] = dout * act'(out) * ratio[r]; act' is taken from the activation's OUTPUT (> 0: 1, else 0 / slope)."""
    g = f64(dout)
    if act != ACT_NONE:
        o = f64(out)
        g = g * np.where(o > 0, 1.0, 0.0 if act == ACT_RELU else slope)
    if ratio is not None:
        g = g * f64(ratio).reshape(-1, 1)
    return g
