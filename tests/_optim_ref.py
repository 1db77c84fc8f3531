"""fp64 evaluation of what mdm_optim_update computes (csrc/optim.hip, include/mdm_hip.h), its error bounds, and the planted faults.

`ref_update` evaluates the formulas of the header in fp64 on the kernel's own fp32 inputs -- tensors AND the 8-float hyper-parameter
block, whose fp32 values are the kernel's hyper-parameters (fp32(0.999) is not 0.999: 1 - beta2 differs by 1.3e-5 between the two).
Next to every result it returns `mag`: the same expression over absolute values, the scale rounding errors are measured in.

SGD bound, by counting fp32 roundings (u = 2^-24 each; a fused multiply-add only removes one).  Clip coefficient: sqrtf, * gmul, the
constant 1e-6f, +, /, coef * c = 6.  Then
    buf :  6 + (coef g, wd p, +) 3 + (buf_decay buf, g_scale d, +) 3                               = 12   in  mag(buf)
    p   :  12 + (momentum buf, +) 2 + (lr d, p -) 2                                               = 16   in  |p| + lr mag(update)
    ema :  the bound of p + (1 - d, e - p, *, e -) 4                                              in  |e| + (1 - d)(|e| + |p_new|)
Adam's moments are plain arithmetic too:
    m   :  6 + 3 + (1 - beta1, * d, beta1 m, +) 4                                                 = 13   in  mag(m)
    v   :  2 x 9 (d twice) + (1 - beta2, * d, * d, beta2 v, +) 5                                  = 23   in  mag(v)
AdamW (kind 3) is Adam with the decay moved: p (1 - lr wd) in front of the moments instead of wd p inside d.  Its moments see one
term less and keep Adam's counts as upper bounds; the product adds two roundings to the parameter's chain, which the CPU figure of
torch.optim.AdamW carries.
Adam's parameter goes through sqrtf, rsqrtf and a division whose errors under the build's flags are not documented: its bound is
4 x the error torch.optim.Adam (AdamW for kind 3) itself makes on the CPU in fp32 (`adam_cpu_figure`), both being fp32 chains of the same length.
None of this depends on the data.
"""
import functools
import math

import torch

U = 2.0 ** -24
SGD, SGD_M, ADAM, ADAMW = 0, 1, 2, 3
R_SGD_BUF, R_SGD_P, R_EMA, R_ADAM_M, R_ADAM_V = 12, 16, 4, 13, 23

# name -> (kind, lr, keyword hyper-parameters): the variants the tests cover
VARIANTS = {
    "sgd": (SGD, 0.1, {}),
    "sgd_momentum_dampening_wd": (SGD_M, 0.1, dict(momentum=0.9, dampening=0.5, weight_decay=0.1)),
    "sgd_nesterov": (SGD_M, 0.1, dict(momentum=0.9, nesterov=True)),
    "adam": (ADAM, 1e-3, {}),
    "adam_wd": (ADAM, 1e-2, dict(weight_decay=0.1)),       # lr 1e-2: decoupled-instead-of-coupled then shows at 1e-3 |p|
    "adamw": (ADAMW, 1e-3, dict(weight_decay=1e-2)),       # torch's default decay
    "adamw_wd": (ADAMW, 1e-2, dict(weight_decay=0.1)),     # ... and coupled-instead-of-decoupled does
}
# (sqnorm, max_norm, gmul): the clip is active in the first two (norm 2.5 -> c = 0.4; 1.25 -> 0.8), inactive in the next two (c >= 1),
# and switched off in the last (max_norm <= 0: the squared norm is not read)
CLIPS = [(6.25, 1.0, 1.0), (6.25, 1.0, 0.5), (0.25, 1.0, 1.0), (0.25, 1.0, 0.5), (6.25, 0.0, 0.5)]


def rbound(r):
    return (1.0 + U) ** r - 1.0


def hp_block(kind, step, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, betas=(0.9, 0.999), eps=1e-8,
             ema_decay=0.0, first_step_rule=True, keep_dampening=True):
    """The 8 floats the host sends for the optimizer's step `step` (1-based), fp32.  Planted faults: `first_step_rule=False`,
    `keep_dampening=False`."""
    if kind >= ADAM:
        b1, b2 = (float(torch.tensor(b, dtype=torch.float32)) for b in betas)      # what the block holds
        h = [lr, b1, b2, eps, weight_decay, 1 - b1 ** step, 1 - b2 ** step, ema_decay]
    else:
        first = kind == SGD or (step == 1 and first_step_rule)
        damp = dampening if keep_dampening else 0.0
        h = [lr, momentum, 0.0 if first else momentum, 1.0 if first else 1.0 - damp, weight_decay, float(nesterov), 0.0, ema_decay]
    return torch.tensor(h, dtype=torch.float32)


def coef64(sqnorm, max_norm, gmul, wrong=None):
    coef = gmul
    if max_norm > 0:
        norm = math.sqrt(sqnorm) * (1.0 if wrong == "gmul_after_clip_test" else gmul)
        c = max_norm / (norm + 1e-6)
        if c < 1.0:
            coef *= c
    return coef


def ref_update(kind, hp, p, g, s0, s1, ema, sqnorm, max_norm, gmul, wrong=None):
    """One update in fp64.  p, g, s0, s1, ema: fp32 tensors (or None) on any device; hp: the fp32 block.
    -> dict name -> (value, mag) for p, s0, s1, ema (those that exist).  `wrong`: a planted fault."""
    h = [float(x) for x in hp.double().cpu()]
    ed = h[7]
    p, g = p.double(), g.double()
    coef = coef64(float(sqnorm), float(max_norm), float(gmul), wrong)
    out = {}
    if kind >= ADAM:
        lr, b1, b2, eps, wd, bc1, bc2 = h[:7]
        m0, v0 = s0.double(), s1.double()
        if (kind == ADAMW and wrong != "coupled_decay") or wrong == "decoupled_decay":
            p_in, d, D = p * (1.0 - lr * wd), coef * g, (coef * g).abs()
        else:
            p_in, d, D = p, coef * g + wd * p, (coef * g).abs() + wd * p.abs()
        m, M = b1 * m0 + (1 - b1) * d, b1 * m0.abs() + (1 - b1) * D
        v, V = b2 * v0 + (1 - b2) * d * d, b2 * v0 + (1 - b2) * D * D
        denom = v.sqrt() / math.sqrt(bc2) + eps
        p_new, P = p_in - (lr / bc1) * m / denom, p.abs() + (lr / bc1) * M / denom
        out["s0"], out["s1"] = (m, M), (v, V)
    else:
        lr, mom, bd, gs, wd, nes = h[:6]
        d, D = coef * g + wd * p, (coef * g).abs() + wd * p.abs()
        if kind == SGD_M:
            b0 = s0.double()
            b, B = bd * b0 + gs * d, bd * b0.abs() + gs * D
            if nes:
                d, D = d + mom * (b0 if wrong == "nesterov_old_buffer" else b), D + mom * B
            else:
                d, D = b, B
            out["s0"] = (b, B)
        p_new, P = p - lr * d, p.abs() + lr * D
    out["p"] = (p_new, P)
    if ema is not None:
        e = ema.double()
        out["ema"] = (e - (1 - ed) * (e - p_new), e.abs() + (1 - ed) * (e.abs() + p_new.abs()))
    return out


def inputs(n, seed=0, device="cpu"):
    """p, g, s0 (a momentum buffer / first moment), s1 (a second moment), ema: fp32, O(1), some |p| near 0."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(n, generator=gen)
    p, g, s0, s1, e = r(), r(), 0.3 * r(), 0.1 * r() ** 2, r()
    p[::7] *= 1e-3
    return [t.to(device) for t in (p, g, s0, s1, e)]


def _torch_adam_step(kind, p, g, m, v, step, hp, sqnorm, max_norm, gmul):
    """torch.optim.Adam (AdamW for kind 3) on the CPU in fp32 from the given state, behind torch's clip_grad_norm_ arithmetic (with
    the norm given)."""
    h = [float(x) for x in hp.double()]
    g = g * torch.tensor(gmul, dtype=torch.float32)
    if max_norm > 0:
        norm = torch.tensor(sqnorm, dtype=torch.float32).sqrt() * torch.tensor(gmul, dtype=torch.float32)
        g = g * torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    P = torch.nn.Parameter(p.clone())
    opt = (torch.optim.AdamW if kind == ADAMW else torch.optim.Adam)([P], lr=h[0], betas=(h[1], h[2]), eps=h[3], weight_decay=h[4], foreach=False)
    opt.state[P] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    P.grad = g
    opt.step()
    st = opt.state[P]
    return P.detach(), st["exp_avg"], st["exp_avg_sq"]


@functools.lru_cache(maxsize=None)
def adam_cpu_figure(name, n=1 << 16, steps=3):
    """Largest |p - p64| / (u mag) torch.optim.Adam (AdamW for kind 3) makes in fp32 on the CPU over `steps` steps from zero moments and every clip case,
    each step against the fp64 evaluation from torch's own state before it."""
    kind, lr, kw = VARIANTS[name]
    assert kind >= ADAM
    worst = 0.0
    for sq, mx, gm in CLIPS:
        p, g0, _, _, _ = inputs(n, seed=5)
        m, v = torch.zeros(n), torch.zeros(n)
        for k in range(1, steps + 1):
            g = torch.roll(g0, k)
            hp = hp_block(kind, k, lr, **kw)
            want, mag = ref_update(kind, hp, p, g, m, v, None, sq, mx, gm)["p"]
            p, m, v = _torch_adam_step(kind, p, g, m, v, k, hp, sq, mx, gm)
            worst = max(worst, float(((p.double() - want).abs() / (U * mag)).max()))
    return worst


def bounds(name, ref):
    """name of a variant, ref = ref_update(...) -> dict name -> per-element absolute bound."""
    kind = VARIANTS[name][0]
    tiny = 2.0 ** -140
    if kind >= ADAM:
        b = {"p": 4.0 * adam_cpu_figure(name) * U * ref["p"][1], "s0": rbound(R_ADAM_M) * ref["s0"][1], "s1": rbound(R_ADAM_V) * ref["s1"][1]}
    else:
        b = {"p": rbound(R_SGD_P) * ref["p"][1]}
        if kind == SGD_M:
            b["s0"] = rbound(R_SGD_BUF) * ref["s0"][1]
    if "ema" in ref:
        b["ema"] = b["p"] + rbound(R_EMA) * ref["ema"][1]
    return {k: v + tiny for k, v in b.items()}


# planted fault -> (variant it is planted in, (sqnorm, max_norm, gmul), hp_block keywords, ref_update's `wrong`)
CONTROLS = {
    "no_first_step_rule": ("sgd_momentum_dampening_wd", CLIPS[0], dict(first_step_rule=False), None),
    "dampening_dropped": ("sgd_momentum_dampening_wd", CLIPS[0], dict(keep_dampening=False), None),
    "nesterov_old_buffer": ("sgd_nesterov", CLIPS[0], {}, "nesterov_old_buffer"),
    "decoupled_decay": ("adam_wd", CLIPS[0], {}, "decoupled_decay"),
    "coupled_decay": ("adamw_wd", CLIPS[0], {}, "coupled_decay"),
    # norm 1.5, gmul 0.5: the averaged gradient (0.75) is inside the ball, the summed one is not
    "gmul_after_clip_test": ("sgd", (2.25, 1.0, 0.5), {}, "gmul_after_clip_test"),
}


def trajectory(name, clip, n=4096, steps=3, hp_kw=None, wrong=None):
    """`steps` updates in fp64 from zero state (each step's inputs rounded to fp32, as the kernel's are) -> (p, bound of the last step)."""
    kind, lr, kw = VARIANTS[name]
    sq, mx, gm = clip
    p, g0, _, _, _ = inputs(n, seed=9)
    s0, s1 = torch.zeros(n), torch.zeros(n)
    for k in range(1, steps + 1):
        hp = hp_block(kind, k, lr, **dict(kw, **(hp_kw or {})))
        ref = ref_update(kind, hp, p, torch.roll(g0, k), s0, s1, None, sq, mx, gm, wrong)
        last = ref
        p = ref["p"][0].float()
        s0 = ref["s0"][0].float() if "s0" in ref else s0
        s1 = ref["s1"][0].float() if "s1" in ref else s1
    return last["p"][0], bounds(name, last)["p"]
