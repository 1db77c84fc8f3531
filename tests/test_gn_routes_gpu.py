"""Every GroupNorm route (csrc/norm.hip: gn_route) on the GPU.  Each row names the forward and backward kernel it expects per
storage type (mdm_gn_route_of before, mdm_gn_last_route after each launch), is held against F.group_norm (+ SiLU) and its autograd
with the tolerances of test_kernels_gpu.test_groupnorm_fwd_bwd, and must repeat itself bit for bit on a second launch.  The rows
are the smallest at which each rung of the vectors-per-lane ladder, the widened fp32 block and the generic kernels are taken."""
import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import DT, _dev, _q, _relerr, _tol, _up

pytestmark = pytest.mark.gpu

N, G = 2, 32
# (C0, C1, P): {storage type: (forward route, backward route)}
ROWS = {
    (32, 0, 64): {"bf16": ("fwd_reg<1,256>", "bwd_reg<1,256>"), "f32": ("fwd_reg<1,256>", "bwd+reduce")},
    (32, 0, 128): {"bf16": ("fwd_reg<2,256>", "bwd_reg<2,256>"), "f32": ("fwd_reg<2,256>", "bwd+reduce")},
    (32, 0, 256): {"bf16": ("fwd_reg<2,512>", "bwd_reg<2,512>"), "f32": ("fwd_reg<2,512>", "bwd+reduce")},
    # 16-channel blocks above 256 pixels; the fp32 forward widens them to 32 while the slice still fits the registers
    (32, 0, 576): {"bf16": ("fwd_reg<4,512>", "bwd_reg<4,512>"), "f32": ("fwd_reg<8,512>", "bwd+reduce")},
    (32, 0, 2048): {"bf16": ("fwd_reg<8,512>", "bwd_reg<8,512>"), "f32": ("fwd_reg<8,512>", "bwd+reduce")},
    (32, 0, 4096): {"bf16": ("fwd", "bwd"), "f32": ("fwd", "bwd+reduce")},      # 32 vectors per lane: the streaming kernels
    (64, 32, 64): {"bf16": ("fwd_reg<2,256>", "bwd_reg<2,256>"), "f32": ("fwd_reg<2,256>", "bwd+reduce")},      # two sources, 48-channel blocks
}
CASES = [(dt, row) for row in ROWS for dt in ("f32", "bf16")]


def test_rows_reach_every_route():
    from mdm import _lib
    assert {r for per_dt in ROWS.values() for pair in per_dt.values() for r in pair} == set(_lib.gn_route_names())


@pytest.mark.parametrize("dt,row", CASES, ids=[f"{dt}-{'+'.join(map(str, row))}" for dt, row in CASES])
def test_route_parity_and_repeatability(dt, row):
    from mdm import _lib, ops
    C0, C1, P = row
    fwd, bwd = ROWS[row][dt]
    C, silu = C0 + C1, P != 576
    shape = dict(dtype=DT[dt], N=N, P=P, G=G, C0=C0, C1=C1)
    g = torch.Generator().manual_seed(C + P)
    x = _q(torch.randn(N, C, P, generator=g) * 1.5 + 0.3, dt).requires_grad_(True)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=g)).requires_grad_(True)
    y = F.group_norm(x, G, gamma, beta, eps=1e-6)
    if silu:
        y = F.silu(y)
    gy = _q(torch.randn(y.shape, generator=g), dt)
    y.backward(gy)
    xg = x.detach().view(N, G, -1)
    want_stats = torch.stack((xg.mean(2), (xg.var(2, unbiased=False) + 1e-6).rsqrt()), 2)
    dev = _dev()
    xh = x.detach().permute(0, 2, 1).contiguous()          # [N, P, C]
    s0 = _up(xh[..., :C0], dt)
    s1 = _up(xh[..., C0:], dt) if C1 else None
    gyh = _up(gy.permute(0, 2, 1), dt)
    gd, bd = gamma.detach().to(dev), beta.detach().to(dev)
    ws = torch.empty(_lib.load().mdm_groupnorm_bwd_ws_floats(DT[dt], N, C) or 1, device=dev)
    runs = []
    for _ in range(2):
        out = torch.full((N, P, C), float("nan"), device=dev, dtype=s0.dtype)
        stats = torch.full((N, G, 2), float("nan"), device=dev)
        assert _lib.gn_route_of(0, **shape) == fwd
        ops.groupnorm_fwd(DT[dt], s0, C0, s1, C1, N, P, gd, bd, silu, out, stats, ws)
        assert _lib.gn_last_route() == fwd
        d0 = torch.full_like(s0, float("nan"))
        d1 = torch.full_like(s1, float("nan")) if C1 else None
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        assert _lib.gn_route_of(1, **shape) == bwd
        ops.groupnorm_bwd(DT[dt], s0, C0, s1, C1, N, P, gd, bd, silu, gyh, stats, d0, 0, d1, 0, dg, db, ws)
        assert _lib.gn_last_route() == bwd
        torch.cuda.synchronize()
        runs.append((out, stats, d0 if d1 is None else torch.cat((d0, d1), 2), dg, db))
    out, stats, dx, dg, db = runs[0]
    errs = dict(y=_relerr(out, y.detach().permute(0, 2, 1)), stats=_relerr(stats, want_stats), dx=_relerr(dx, x.grad.permute(0, 2, 1)),
                dgamma=_relerr(dg, gamma.grad), dbeta=_relerr(db, beta.grad))
    print(dt, row, errs)
    # (the statistics are fp32 sums over inputs both sides hold exactly, whatever the storage type: the fp32 tolerance)
    assert errs["y"] < _tol(dt, 0.5) and errs["stats"] < _tol("f32") and errs["dx"] < _tol(dt)
    assert errs["dgamma"] < _tol(dt, 0.25) and errs["dbeta"] < _tol(dt, 0.25)
    # every sum inside a workgroup has a fixed order; bf16 dgamma / dbeta meet across the images in float atomics
    same = [torch.equal(a, b) for a, b in zip(*runs)]
    assert all(same[:3]), same
    if dt == "f32":
        assert all(same[3:]), same


def test_a_refused_descriptor_launches_nothing():
    from mdm import _lib, ops
    dev = _dev()
    C, P = 40, 16                      # 40 channels do not divide into 32 groups
    s0 = torch.zeros(N, P, C, device=dev)
    y = torch.full((N, P, C), float("nan"), device=dev)
    stats = torch.full((N, G, 2), float("nan"), device=dev)
    gd = torch.ones(C, device=dev)
    ops.groupnorm_fwd(DT["f32"], torch.zeros(N, P, 32, device=dev), 32, None, 0, N, P, gd, gd, 1, torch.empty(N, P, 32, device=dev),
                      torch.empty(N, G, 2, device=dev), None)
    assert _lib.gn_last_route() == "fwd_reg<1,256>"
    assert _lib.gn_route_of(0, dtype=DT["f32"], N=N, P=P, G=G, C0=C, C1=0) is None
    with pytest.raises(RuntimeError, match="not divisible by G"):
        ops.groupnorm_fwd(DT["f32"], s0, C, None, 0, N, P, gd, gd, 1, y, stats, None)
    torch.cuda.synchronize()
    assert _lib.gn_last_route() == "none"
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(stats).all())
