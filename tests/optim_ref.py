"""The optimiser kernels' yardstick: one Adam / AdamW step in numpy fp64, the same step by torch.optim on the CPU, the value
regimes every arena is filled with, and the criterion that holds a kernel to both.

k_adam (ConvAE, and the VAE through its trunk) and k_adam_l2 (Linear) are torch.optim.Adam with L2 weight decay, k_adamw (UNET)
is torch.optim.AdamW; all three are element-wise, so a test may write any (p, g, m, v) it likes into an engine's arenas, take
one step at any step number and compare element by element (tests/test_optim_elementwise_gpu.py).  No GPU is needed here.
"""
import numpy as np

REGIMES = ("typical", "zero_state", "eps_dominated", "no_gradient", "large", "small_weight")
QUANTITIES = ("update", "exp_avg", "exp_avg_sq")

# hyper set -> (settings, the step numbers t it is taken at); t is the number of the step being taken
HYPERS = {
    "default": (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=1e-5), (1, 2, 10, 1000, 100000)),
    "strong": (dict(lr=3e-2, betas=(0.5, 0.9), eps=1e-3, wd=0.1), (1, 7)),
    "no_decay": (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0), (3,)),
    "beta1_zero": (dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, wd=1e-5), (1, 5)),
}
CASES = [(name, t) for name, (_, steps) in HYPERS.items() for t in steps]


def _f64(*arrays):
    return tuple(np.asarray(a, dtype=np.float64) for a in arrays)


def adam_l2_f64(p, g, m, v, t, lr, betas, eps, wd):
    """torch.optim.Adam, single-tensor formula, step number t >= 1: (p_new, m_new, v_new) in fp64"""
    (p, g, m, v) = _f64(p, g, m, v)
    (b1, b2) = betas
    if wd != 0:
        g = g + wd * p                              # grad.add(param, alpha=weight_decay)
    w = 1.0 - b1                                    # exp_avg.lerp_(grad, 1 - beta1), the form of ATen's lerp for each weight
    m = m + w * (g - m) if w < 0.5 else g - (g - m) * (1.0 - w)
    v = v * b2 + (1.0 - b2) * g * g                 # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    step_size = lr / (1.0 - b1 ** t)
    denom = np.sqrt(v) / (1.0 - b2 ** t) ** 0.5 + eps
    return p - step_size * (m / denom), m, v


def adamw_f64(p, g, m, v, t, lr, betas, eps, wd):
    """torch.optim.AdamW, single-tensor formula: the decay multiplies the weight, the gradient is left alone"""
    (p, g, m, v) = _f64(p, g, m, v)
    (p_new, m, v) = adam_l2_f64(p * (1.0 - lr * wd), g, m, v, t, lr, betas, eps, 0.0)
    return p_new, m, v


F64 = {"adam": adam_l2_f64, "adamw": adamw_f64}


def torch_step(kind, dtype, p, g, m, v, t, lr, betas, eps, wd):
    """the same step by torch.optim.Adam ("adam") or torch.optim.AdamW ("adamw"), foreach=False, on CPU tensors of `dtype`
    ("float32": the reference with its own error; "float64": a cross-check of the numpy formulas).  Numpy (p_new, m_new, v_new)."""
    import torch
    dt = getattr(torch, dtype) if isinstance(dtype, str) else dtype
    mk = lambda a: torch.tensor(np.asarray(a), dtype=dt)
    w = torch.nn.Parameter(mk(p))
    cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[kind]
    opt = cls([w], lr=lr, betas=tuple(betas), eps=eps, weight_decay=wd, foreach=False)
    opt.state[w] = {"step": torch.tensor(float(t - 1)), "exp_avg": mk(m), "exp_avg_sq": mk(v)}
    w.grad = mk(g)
    opt.step()
    st = opt.state[w]
    assert float(st["step"]) == float(t)
    return w.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()


def regimes(n, seed):
    """(regime, p, g, m, v): regime[i] = i % 6 indexes REGIMES - every tensor, every group of four and every workgroup of an
    arena holds all six - and the fp32 arrays of a step's inputs.  Every non-zero |g| is at least 1e-15, so g * g stays a normal
    fp32 number."""
    rng = np.random.default_rng(seed)
    regime = (np.arange(n) % len(REGIMES)).astype(np.int8)
    is_ = lambda name: regime == REGIMES.index(name)
    g = rng.normal(0.0, 1e-2, n)
    noise = rng.normal(0.0, 1e-3, n)
    spread = rng.uniform(0.5, 1.5, n)
    p = rng.normal(0.0, 0.1, n)
    scale = np.ones(n)
    scale[is_("eps_dominated")] = 1e-7
    scale[is_("large")] = 1e5                       # g ~ 1e3, v ~ 1e6
    g = g * scale
    g = np.where(np.abs(g) < 1e-15, np.where(g < 0, -1e-15, 1e-15), g)
    m = 0.1 * g + noise * scale
    v = g * g * spread
    p[is_("small_weight")] *= 1e-3
    g[is_("no_gradient")] = 0.0
    for a in (p, m, v):
        a[is_("zero_state")] = 0.0
    return (regime,) + tuple(a.astype(np.float32) for a in (p, g, m, v))


def typical(n, seed):
    """(p, g, m, v) of n elements, all of the `typical` regime of regimes(6 n, seed): moments for a step that runs a model"""
    (regime, *arrays) = regimes(len(REGIMES) * n, seed)
    return tuple(a[regime == 0] for a in arrays)


def criterion(got, ref32, ref64, regime_mask, p_old):
    """One regime (regime_mask: bool over the arena) of one step.  got, ref32, ref64: (p_new, m_new, v_new) of the kernel, of
    torch in fp32 and of the fp64 formula, all from the same fp32 inputs.  Per quantity - the update p_new - p_old, exp_avg,
    exp_avg_sq - with the maxima over the regime's elements:

        max|got - f64| <= 3 max|ref32 - f64| + 2^-21 max|f64|  (+ 2^-24 max|p_old| for the update)

    3 is the project's factor (helpers.assert_close_as_reference); the floor is four fp32 ulps of the regime's largest value,
    for the handful of roundings whose order an FMA contraction may change where the reference happens to be exact; the extra
    term is the half-ulp rounding of the stored weight.  Returns {quantity: (err / bound, arena index of the worst element)}."""
    idx = np.flatnonzero(regime_mask)
    p0 = np.asarray(p_old, dtype=np.float64)[idx]
    out = {}
    for k, name in enumerate(QUANTITIES):
        (a, r, e) = (np.asarray(x[k], dtype=np.float64)[idx] for x in (got, ref32, ref64))
        if k == 0:
            (a, r, e) = (a - p0, r - p0, e - p0)
        err = np.abs(a - e)
        bound = 3.0 * float(np.abs(r - e).max()) + 2.0 ** -21 * float(np.abs(e).max())
        if k == 0:
            bound += 2.0 ** -24 * float(np.abs(p0).max())
        worst = int(np.argmax(np.where(np.isfinite(err), err, np.inf)))
        e_max = float(err[worst])
        ratio = 0.0 if e_max == 0.0 else (e_max / bound if bound > 0 and np.isfinite(e_max) else float("inf"))
        out[name] = (ratio, int(idx[worst]))
    return out


def check_step(got, ref32, ref64, regime, p_old, label, name_of=None, limit=1.0):
    """criterion() over every regime; asserts every ratio <= limit, naming `label` (engine, hyper set, step), regime, quantity,
    arena index and - name_of(index) - the tensor.  Returns {(regime, quantity): ratio}."""
    ratios = {}
    failures = []
    for r, rname in enumerate(REGIMES):
        mask = np.asarray(regime) == r
        if not mask.any():
            continue
        for q, (ratio, i) in criterion(got, ref32, ref64, mask, p_old).items():
            ratios[(rname, q)] = ratio
            if not ratio <= limit:
                k = QUANTITIES.index(q)
                failures.append(f"{label}, {rname}, {q}: {ratio:.3g}x the bound at arena index {i}"
                                f"{' (' + name_of(i) + ')' if name_of else ''}: got {float(got[k][i])!r}, fp32 reference "
                                f"{float(ref32[k][i])!r}, fp64 {float(ref64[k][i])!r}")
    assert not failures, "\n".join(failures)
    return ratios


def emulate_f32(kind, one_minus_beta, p, g, m, v, t, lr, betas, eps, wd):
    """the kernels' arithmetic in numpy fp32 (fmaf as an fp64 product-sum rounded once).  one_minus_beta: "rounded_once" is
    (float)(1.0 - beta), "from_rounded_beta" is 1.f - (float)beta."""
    f = np.float32
    (p, g, m, v) = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(f)
    (b1, b2) = betas
    if one_minus_beta == "rounded_once":
        (o1, o2) = (f(1.0 - b1), f(1.0 - b2))
    else:
        assert one_minus_beta == "from_rounded_beta"
        (o1, o2) = (f(1.0) - f(b1), f(1.0) - f(b2))
    step_size = f(lr / (1.0 - b1 ** t))
    bc2_sqrt = f((1.0 - b2 ** t) ** 0.5)
    if kind == "adamw":
        p = p * f(1.0 - lr * wd)
    elif wd != 0:
        g = fma(p, f(wd), g)
    m = m + (g - m) * o1 if o1 < 0.5 else g - (g - m) * (f(1.0) - o1)      # adam_lerp
    v = fma(g * g, o2, v * f(b2))
    denom = np.sqrt(v) / bc2_sqrt + f(eps)
    return p - step_size * (m / denom), m, v
