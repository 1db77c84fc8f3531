"""CPU self-test of the error-bound checker (tests/_bounds.py): it accepts a correctly rounded bf16 convolution and rejects
each planted fault a wrong kernel could make -- a dropped tap at one border pixel, a dropped 32-channel K-chunk, the rowvec of
the neighbouring image on one tile, truncation instead of round-to-nearest-even, a write one past the end, a NaN left in an
overwrite destination, an ignored acc1."""
import pytest
import torch

from _bounds import Buf, check, conv_dgrad_ref, conv_fwd_ref, epilogue_ref, rne_bf16, trunc_bf16

N, H, C, CO, TAPS = 3, 8, 64, 32, 9
PADS = (1, 1, 1, 1)


def _problem():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, H, H, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(TAPS, CO, C, generator=g) / (TAPS * C) ** 0.5).to(torch.bfloat16)
    bias = torch.randn(CO, generator=g)
    rv_ld, rv_off = CO + 16, 8
    rv = torch.randn(N * rv_ld + rv_off, generator=g)
    acc, mag = conv_fwd_ref(x, None, w, 3, 3, 1, PADS, 0)
    ref, mg = epilogue_ref(acc.reshape(-1, CO), mag.reshape(-1, CO), bias=bias, rowvec=rv, rv_ld=rv_ld, rv_off=rv_off,
                           rows_per_img=H * H)
    return x, w, bias, rv, rv_ld, rv_off, ref, mg


def _ok(y, ref, mg):
    check("conv", y, ref, mg, TAPS * C, "bf16")


def test_accepts_correctly_rounded_result():
    *_, ref, mg = _problem()
    ratio, rel = check("conv", rne_bf16(ref), ref, mg, TAPS * C, "bf16")
    assert ratio <= 1.0 and 5e-4 < rel < 3e-3


def test_rejects_dropped_tap_at_border_pixel():
    x, w, *_, ref, mg = _problem()
    y = ref.clone()
    # output pixel (image 1, row 0, col 0): drop tap (1, 1) -- the centre tap, input pixel (0, 0)
    contrib = x[1, 0, 0].double() @ w[4].double().t()
    y[1 * H * H + 0] -= contrib
    with pytest.raises(AssertionError, match="outside the bound"):
        _ok(rne_bf16(y), ref, mg)


def test_rejects_dropped_k_chunk():
    x, w, *_, ref, mg = _problem()
    xz = x.clone()
    xz[..., 32:64] = 0          # channels 32..63 of every tap missing, on the first 64-pixel tile only
    acc, _ = conv_fwd_ref(xz, None, w, 3, 3, 1, PADS, 0)
    full, _ = conv_fwd_ref(x, None, w, 3, 3, 1, PADS, 0)
    y = ref.clone()
    y[:64] += (acc - full).reshape(-1, CO)[:64]
    with pytest.raises(AssertionError, match="outside the bound"):
        _ok(rne_bf16(y), ref, mg)


def test_rejects_rowvec_of_neighbouring_image():
    x, w, bias, rv, rv_ld, rv_off, ref, mg = _problem()
    y = ref.clone()
    tile = slice(2 * H * H, 2 * H * H + 32)       # one 32-pixel tile of the last image takes image 1's rowvec
    y[tile] += (rv[rv_off + 1 * rv_ld:rv_off + 1 * rv_ld + CO] - rv[rv_off + 2 * rv_ld:rv_off + 2 * rv_ld + CO]).double()
    with pytest.raises(AssertionError, match="outside the bound"):
        _ok(rne_bf16(y), ref, mg)


def test_rejects_truncation_instead_of_rne():
    *_, ref, mg = _problem()
    with pytest.raises(AssertionError, match="outside the bound"):
        _ok(trunc_bf16(ref), ref, mg)


def test_rejects_write_one_past_the_end():
    *_, ref, mg = _problem()
    b = Buf(ref.shape, torch.bfloat16, "cpu", rne_bf16(ref))
    assert b.guards_intact()
    b.raw[b.g + b.n] = 0.0          # the element after the last one
    assert not b.guards_intact()
    assert b.first_bad_guard() == (None, b.n)


def test_rejects_nan_left_in_overwrite_destination():
    *_, ref, mg = _problem()
    b = Buf(ref.shape, torch.bfloat16, "cpu")        # NaN-prefilled
    b.t.copy_(rne_bf16(ref))
    b.t[37, 5] = float("nan")                          # one element the kernel did not write
    with pytest.raises(AssertionError, match="non-finite"):
        _ok(b.t, ref, mg)


def test_rejects_ignored_acc1():
    """Data gradient into split destinations, acc0 = 0, acc1 = 1: D1 written as if acc1 were 0."""
    g = torch.Generator().manual_seed(6)
    C0, C1 = 32, 32
    dy = torch.randn(N, H, H, CO, generator=g).to(torch.bfloat16)
    w = (torch.randn(TAPS, CO, C0 + C1, generator=g) / (TAPS * CO) ** 0.5).to(torch.bfloat16)
    prior1 = torch.randn(N * H * H, C1, generator=g).to(torch.bfloat16)
    a, m = conv_dgrad_ref(dy, w, H, H, C0 + C1, 3, 3, 1, PADS)
    ref1, mg1 = epilogue_ref(a[..., C0:].reshape(-1, C1), m[..., C0:].reshape(-1, C1), prior=prior1)
    check("d1", rne_bf16(ref1), ref1, mg1, TAPS * CO, "bf16")
    no_acc, _ = epilogue_ref(a[..., C0:].reshape(-1, C1), m[..., C0:].reshape(-1, C1))
    with pytest.raises(AssertionError, match="outside the bound"):
        check("d1", rne_bf16(no_acc), ref1, mg1, TAPS * CO, "bf16")
