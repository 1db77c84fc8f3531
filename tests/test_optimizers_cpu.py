"""SGD and Adam next to AdamW (`--optim {adam, adamw, sgd}`, reference main_train_masked.py:134-141, 375), host side: the C ABI
entry, the classes' argument checks and torch.optim state-dict grammar, `get_optimizer`, and -- in fp64, no device needed -- that the
bounds of tests/test_optimizers_gpu.py would catch each planted fault.  No kernel is launched."""
import os
import re

import pytest
import torch

import _optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_bound_and_exported():
    from mdm import _lib
    header = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    declared = set(re.findall(r"\b(mdm_[a-z0-9_]+)\s*\(", header))
    assert "mdm_optim_update" in declared and "mdm_optim_update" in _lib.EXPORTS
    assert "mdm_adamw_ema" not in header and "mdm_adamw_ema" not in _lib.EXPORTS      # AdamW is kind 3 of the one entry point
    args, res = _lib._PROTOS["mdm_optim_update"]
    assert len(args) == 13 and args[0] is _lib.i32 and args[7] is _lib.i64 and args[10] is args[11] is _lib.f32 and res is _lib.i32
    lib = _lib.load()
    fn = lib.mdm_optim_update
    # argument checks run before any launch: a bad kind, a missing state buffer, a misaligned buffer
    assert fn(4, 16, 16, None, None, None, None, 8, 16, None, 0.0, 1.0, None) != 0 and b"kind" in lib.mdm_last_error()
    assert fn(1, 16, 16, None, None, None, None, 8, 16, None, 0.0, 1.0, None) != 0 and b"state buffer" in lib.mdm_last_error()
    assert fn(2, 16, 16, 16, None, None, None, 8, 16, None, 0.0, 1.0, None) != 0 and b"both" in lib.mdm_last_error()
    assert fn(3, 16, 16, 16, None, None, None, 8, 16, None, 0.0, 1.0, None) != 0 and b"both" in lib.mdm_last_error()
    assert fn(0, 20, 16, None, None, None, None, 8, 16, None, 0.0, 1.0, None) != 0 and b"aligned" in lib.mdm_last_error()
    assert fn(0, 16, 16, None, None, None, None, 8, 16, None, 1.0, 1.0, None) != 0 and b"squared norm" in lib.mdm_last_error()


class _Store:
    """The part of mdm.unet.ParamStore the optimizers touch, on the host (a real store needs a device)."""

    def __init__(self, n=64):
        self.P, self.G, self.Pb, self.size = torch.zeros(n), torch.zeros(n), None, n

    def state_dict(self, order=None, src=None):
        return {"w": (self.P if src is None else src).clone()}

    def flat_from_reference(self, sd):
        return sd["w"].reshape(-1)


class _Model:
    def __init__(self):
        self.store = _Store()

    def reference_param_order(self):
        return ["w"]


@pytest.fixture(scope="module")
def model():
    return _Model()


def test_get_optimizer_names_defaults_and_failure(model):
    import mdm
    for name, cls in (("sgd", mdm.SGD), ("SGD", mdm.SGD), ("adam", mdm.Adam), ("Adam", mdm.Adam), ("adamw", mdm.AdamW), ("AdamW", mdm.AdamW)):
        o = mdm.get_optimizer(model, name, 3e-4)
        assert type(o) is cls and o.param_groups[0]["lr"] == 3e-4 and o.param_groups[0]["initial_lr"] == 3e-4
    ref = [torch.nn.Parameter(torch.zeros(1))]
    for ours, theirs in ((mdm.SGD(model, lr=0.1), torch.optim.SGD(ref, lr=0.1)), (mdm.Adam(model, lr=0.1), torch.optim.Adam(ref, lr=0.1)),
                         (mdm.AdamW(model, lr=0.1), torch.optim.AdamW(ref, lr=0.1))):
        want = {k: v for k, v in theirs.state_dict()["param_groups"][0].items() if k != "params"}
        got = {k: v for k, v in ours.state_dict()["param_groups"][0].items() if k not in ("params", "initial_lr")}
        assert got == want and list(got) == list(want), (got, want)               # torch's defaults, torch's fields, torch's order
        assert ours.state_dict()["state"] == {}
    with pytest.raises(UnboundLocalError):                                        # upstream: `optimizer` is never bound
        mdm.get_optimizer(model, "rmsprop", 1e-3)
    assert mdm.SGD(model, lr=0.1).buf is None, "momentum == 0 allocates no state"
    acc = mdm.Accelerator(device="cpu")
    for name in ("sgd", "adam", "adamw"):
        o = mdm.get_optimizer(model, name, 1e-3)
        acc.prepare(model, o)
        assert acc._ckpt["optimizer"] is o


def test_arguments_torch_refuses_are_refused(model):
    import mdm
    bad_sgd = [dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-0.1), dict(dampening=-0.1), dict(nesterov=True),
               dict(nesterov=True, momentum=0.9, dampening=0.1), dict(maximize=True)]
    for kw in bad_sgd:
        with pytest.raises(ValueError):
            mdm.SGD(model, **dict(dict(lr=0.1), **kw))
    for kw in (dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1), dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):                                           # ... and torch does refuse them
            torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], **dict(dict(lr=0.1), **kw))
    bad_adam = [dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-0.1),
                dict(amsgrad=True), dict(maximize=True)]
    for kw in bad_adam:
        with pytest.raises(ValueError):
            mdm.Adam(model, **kw)
    o = mdm.SGD(model, lr=0.1)
    sd = mdm.SGD(model, lr=0.1, momentum=0.9).state_dict()
    with pytest.raises(ValueError, match="momentum"):
        o.load_state_dict(sd)


def test_sgd_block_carries_the_first_step_rule(model):
    import mdm
    o = mdm.SGD(model, lr=0.1, momentum=0.9, dampening=0.5, weight_decay=0.1)
    o.hyper(ema_decay=0.25)
    assert o.hp.tolist() == R.hp_block(R.SGD_M, 1, 0.1, momentum=0.9, dampening=0.5, weight_decay=0.1, ema_decay=0.25).tolist()
    assert o.hp.tolist()[2:4] == [0.0, 1.0]
    o.hyper(ema_decay=0.25)
    assert o.hp.tolist() == R.hp_block(R.SGD_M, 2, 0.1, momentum=0.9, dampening=0.5, weight_decay=0.1, ema_decay=0.25).tolist()
    assert o.hp.tolist()[3] == 0.5
    o.hyper(advance=False)
    assert o.hp.tolist()[2:4] == [torch.tensor(0.9).item(), 0.5] and o.t == 2
    # a loaded momentum buffer is not a first step; a state dict without one is
    o2 = mdm.SGD(model, lr=0.1, momentum=0.9)
    o2.load_state_dict(o.state_dict())
    o2.hyper()
    assert o2.hp.tolist()[2] == torch.tensor(0.9).item() and o2.param_groups[0]["dampening"] == 0.5
    o2.load_state_dict(mdm.SGD(model, lr=0.1, momentum=0.9).state_dict())
    o2.hyper()
    assert o2.hp.tolist()[2:4] == [0.0, 1.0]
    a = mdm.Adam(model, lr=1e-3, weight_decay=0.1)
    a.hyper(); a.hyper(ema_decay=0.5)
    got, want = a.hp.tolist(), R.hp_block(R.ADAM, 2, 1e-3, weight_decay=0.1, ema_decay=0.5).tolist()
    assert got[:5] == want[:5] and got[7] == want[7] and a.t == 2
    # bias corrections: the class takes them from the betas as given, hp_block from the betas the block holds (fp32(0.999) is
    # 1.3e-8 above 0.999, 1.3e-5 of 1 - beta2)
    assert got[5:7] == pytest.approx(want[5:7], rel=1e-4)


@pytest.mark.parametrize("fault", sorted(R.CONTROLS))
def test_planted_faults_clear_100x_the_bound(fault):
    """Each wrong variant, three steps in fp64 on the inputs' distribution of the GPU test, against the right one: more than half of
    the elements differ by more than 100 x the bound the kernel is held to."""
    name, clip, hp_kw, wrong = R.CONTROLS[fault]
    right, bound = R.trajectory(name, clip)
    bad, _ = R.trajectory(name, clip, hp_kw=hp_kw, wrong=wrong)
    ratio = (bad - right).abs() / bound
    assert float((ratio > 100.0).float().mean()) > 0.5, (fault, float(ratio.median()))


def test_adam_cpu_figure_is_a_few_roundings():
    """The yardstick of the Adam and AdamW bounds: torch.optim.Adam's / AdamW's own fp32 error on the CPU, in u = 2^-24 of |p| + lr mag(update).  A chain of
    ~20 roundings cannot honestly sit below half a rounding or above its own length."""
    from _notes import note
    for name in ("adam", "adam_wd", "adamw", "adamw_wd"):
        f = R.adam_cpu_figure(name)
        note("adam_cpu_figure", dict(variant=name, torch_cpu_err_in_u=f, kernel_bound_in_u=4 * f))
        assert 0.5 <= f <= 24.0, (name, f)
