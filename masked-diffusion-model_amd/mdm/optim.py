"""Optimizer-side objects the reference's trainers are handed: AdamW / Adam / SGD, EMA,
LR schedule, and a thin accelerator -- over the flat parameter buffers of mdm.UNet.

Reference call sites: optimizer `get_optimizer(model, args.optim, args.lr)` -> `optim.SGD | Adam | AdamW(model.parameters(), lr=lr)`
(main_train_masked.py:134-141, 375; torch defaults: AdamW betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2; Adam the same with
weight_decay 0; SGD momentum 0, dampening 0, weight_decay 0); EMA `EMAModel(decay=ema_max_decay,
use_ema_warmup=True, inv_gamma, power)` (:116-131) stepped at trainer_masked_mean_shift.py:170-172;
LR schedules diffusers `get_*_schedule_with_warmup` (:144-165).  EMAModel and the LR schedules are
third-party code that is absent from the reference tree: their semantics are implemented from the
call-site arguments and are NOT oracle-checked ("parity unpinned").
"""
from __future__ import annotations

import math

import torch

from . import _lib, ops
from ._lib import call, ptr, stream


class _FlatOptimizer:
    """What AdamW, Adam and SGD share over the flat buffers of a ParamStore: the pinned ring the 8-float hyper-parameter block
    travels through, the squared gradient norm, the launches behind the update kernel, `step` / `zero_grad` / `grad_norm`, and the
    torch.optim `state_dict()` grammar (parameters indexed in `model.reference_param_order()`).  A subclass gives
      _fill(h, g, ema_decay)   write the block for step `self.t` into the pinned slot `h`
      _kernel()                (mdm_optim_update's kind, its first state buffer, its second)
      _state() / _load(st)     the per-parameter `state` entries, out and in
      _group() / _FIELDS       the `param_groups[0]` fields torch writes besides lr / initial_lr / params."""

    def __init__(self, model, group):
        st = model.store
        self.model, self.store = model, st
        self.param_groups = [dict(group, initial_lr=group["lr"])]
        self.t = 0
        # the 8-float hyper-parameter block travels by async H2D copy from pinned memory, which is read when the copy
        # EXECUTES: a host that runs ahead of the GPU must not overwrite a block whose copy has not run yet -> a ring of
        # pinned slots in groups of 16, each group guarded by one event recorded behind its last copy
        self._hp_slots = 64
        self.hp_host = torch.zeros(self._hp_slots, 8).pin_memory() if torch.cuda.is_available() else torch.zeros(self._hp_slots, 8)
        self._hp_events = [None] * (self._hp_slots // 16)
        self._hp_k = 0
        self.hp = torch.zeros(8, device=st.P.device)
        self.sqnorm = torch.zeros(1, device=st.P.device)

    def _advance(self):
        self.t += 1

    _LOAD_REFUSES = ("amsgrad", "maximize", "capturable", "differentiable")      # in a loaded group (AdamW: none, as it always read it)

    def hyper(self, ema_decay=0.0, advance=True):
        """Refresh the 8-float device block the update kernel reads (async H2D)."""
        g = self.param_groups[0]
        if advance:
            self._advance()
        k = self._hp_k
        self._hp_k = (k + 1) % self._hp_slots
        g16 = k // 16
        if k % 16 == 0 and self._hp_events[g16] is not None:
            self._hp_events[g16].synchronize()        # every copy that read this group of slots has executed
        h = self.hp_host[k]
        self._fill(h, g, ema_decay)
        self.hp.copy_(h, non_blocking=True)
        if self.hp.is_cuda and k % 16 == 15:
            ev = self._hp_events[g16] or torch.cuda.Event()
            ev.record()
            self._hp_events[g16] = ev

    def emit_update(self, ema_buf=None, max_norm=1.0, gmul=1.0):
        """Enqueue (or record) grad-norm + clip + update + EMA + bf16 shadow over the flat buffers."""
        st = self.store
        call("mdm_sqnorm", ptr(st.G), st.size, ptr(self.sqnorm), stream())
        kind, buf0, buf1 = self._kernel()
        call("mdm_optim_update", kind=kind, p=ptr(st.P), g=ptr(st.G), buf0=ptr(buf0), buf1=ptr(buf1), ema=ptr(ema_buf),
             shadow_bf16=ptr(st.Pb), n=st.size, hp=ptr(self.hp), sqnorm=ptr(self.sqnorm), max_norm=float(max_norm), gmul=float(gmul),
             stream=stream())
        st.emit_shadows()               # the shadows derived from the weights follow them

    def step(self, max_norm=0.0):
        self.hyper()
        self.emit_update(None, max_norm)

    def zero_grad(self):
        self.store.G.zero_()

    def grad_norm(self):
        return float(self.sqnorm.sqrt())

    def _per_param(self, **bufs):
        """{index: {name: tensor in the reference's shape}} over `model.parameters()` order, from flat buffers."""
        order = self.model.reference_param_order()
        views = {name: self.store.state_dict(order=order, src=b) for name, b in bufs.items()}
        return {i: {name: v[k] for name, v in views.items()} for i, k in enumerate(order)}

    def _flat(self, st, name, dst):
        order = self.model.reference_param_order()
        assert len(st) == len(order), (len(st), len(order))
        dst.copy_(self.store.flat_from_reference({k: st[i][name] for i, k in enumerate(order)}).to(dst.device))

    def state_dict(self):
        g = self.param_groups[0]
        group = dict(lr=g["lr"], **self._group(g), initial_lr=g["initial_lr"], params=list(range(len(self.model.reference_param_order()))))
        return dict(state=self._state(), param_groups=[group])

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        _no(f"{type(self).__name__}.load_state_dict", **{k: g.get(k) for k in self._LOAD_REFUSES})
        new = dict(lr=g["lr"], initial_lr=g.get("initial_lr", g["lr"]))
        for k in self._FIELDS:
            new[k] = tuple(g[k]) if k == "betas" else g[k]
        self._check(new)
        self._load(sd["state"])
        self.param_groups = [new]


def _no(what, **flags):
    for k, v in flags.items():
        if v:
            raise ValueError(f"{what}: {k}=True is not implemented")


def _check_adam(g):
    b1, b2 = g["betas"]
    if not 0.0 <= g["lr"]:
        raise ValueError(f"Invalid learning rate: {g['lr']}")
    if not 0.0 <= g["eps"]:
        raise ValueError(f"Invalid epsilon value: {g['eps']}")
    if not 0.0 <= b1 < 1.0:
        raise ValueError(f"Invalid beta parameter at index 0: {b1}")
    if not 0.0 <= b2 < 1.0:
        raise ValueError(f"Invalid beta parameter at index 1: {b2}")
    if not 0.0 <= g["weight_decay"]:
        raise ValueError(f"Invalid weight_decay value: {g['weight_decay']}")


class _AdamBase(_FlatOptimizer):
    """Two moment buffers, a step count and AdamW's 8-float block: lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2,
    ema_decay.  `torch.optim.Adam[W].state_dict()` layout: per-parameter `step` / `exp_avg` / `exp_avg_sq` in the reference's
    shapes, indexed in `model.parameters()` order (what accelerate writes to optimizer.bin)."""
    _FIELDS = ("betas", "eps", "weight_decay")
    _DECOUPLED = None                   # True: AdamW, mdm_optim_update's kind 3; False: Adam, kind 2

    def __init__(self, model, lr, betas, eps, weight_decay):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.m = torch.zeros_like(self.store.P)
        self.v = torch.zeros_like(self.store.P)

    def _check(self, g):
        pass

    def _kernel(self):
        return (3 if self._DECOUPLED else 2), self.m, self.v

    def _fill(self, h, g, ema_decay):
        b1, b2 = g["betas"]
        h[0] = g["lr"]; h[1] = b1; h[2] = b2; h[3] = g["eps"]
        h[4] = g["weight_decay"]
        h[5] = 1 - b1 ** self.t; h[6] = 1 - b2 ** self.t; h[7] = ema_decay

    def _group(self, g):
        return dict(betas=tuple(g["betas"]), eps=g["eps"], weight_decay=g["weight_decay"], amsgrad=False, maximize=False, foreach=None,
                    capturable=False, differentiable=False, fused=None, decoupled_weight_decay=self._DECOUPLED)

    def _state(self):
        if not self.t:
            return {}
        st = self._per_param(exp_avg=self.m, exp_avg_sq=self.v)
        return {i: dict(step=torch.tensor(float(self.t)), **d) for i, d in st.items()}

    def _load(self, st):
        if st:
            self._flat(st, "exp_avg", self.m)
            self._flat(st, "exp_avg_sq", self.v)
            self.t = int(float(st[0]["step"]))
        else:
            self.m.zero_(); self.v.zero_(); self.t = 0


class AdamW(_AdamBase):
    """`torch.optim.AdamW(params, lr)`: decoupled weight decay (mdm_optim_update, kind 3)."""
    _DECOUPLED = True
    _LOAD_REFUSES = ()

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(model, lr, betas, eps, weight_decay)


class Adam(_AdamBase):
    """`torch.optim.Adam(params, lr)` (main_train_masked.py:137-138): AdamW's moments, bias corrections and step, with the weight
    decay COUPLED -- added to the gradient (L2), so it enters both moments (mdm_optim_update, kind 2)."""
    _DECOUPLED = False

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
        _no("Adam", amsgrad=amsgrad, maximize=maximize)
        _check_adam(dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        super().__init__(model, lr, betas, eps, weight_decay)

    _check = staticmethod(_check_adam)


def _check_sgd(g):
    if g["lr"] < 0.0:
        raise ValueError(f"Invalid learning rate: {g['lr']}")
    if g["momentum"] < 0.0:
        raise ValueError(f"Invalid momentum value: {g['momentum']}")
    if g["dampening"] < 0.0:                     # (torch lets this one through; it has no meaning)
        raise ValueError(f"Invalid dampening value: {g['dampening']}")
    if g["weight_decay"] < 0.0:
        raise ValueError(f"Invalid weight_decay value: {g['weight_decay']}")
    if g["nesterov"] and (g["momentum"] <= 0 or g["dampening"] != 0):
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")


class SGD(_FlatOptimizer):
    """`torch.optim.SGD(params, lr)` (main_train_masked.py:135-136) with torch's momentum / dampening / weight_decay / nesterov
    (mdm_optim_update, kind 0 or 1).  With momentum == 0 there is NO state buffer: two parameter-sized buffers less than AdamW.
    Whether there is one is fixed at construction.  The block: lr, momentum, buf_decay, g_scale, weight_decay, nesterov, 0,
    ema_decay -- (buf_decay, g_scale) = (0, 1) on the step that creates the momentum buffer (torch: buf = d), (momentum,
    1 - dampening) afterwards; it is device memory refreshed per step, so a captured graph follows the rule."""
    _FIELDS = ("momentum", "dampening", "weight_decay", "nesterov")

    def __init__(self, model, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, maximize=False):
        _no("SGD", maximize=maximize)
        g = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        _check_sgd(g)
        super().__init__(model, g)
        self.buf = torch.zeros_like(self.store.P) if momentum != 0 else None
        self._has_buf = False                    # torch: `momentum_buffer` exists from the first step on
        self._first = True                       # the block of the current step carries the first-step rule

    def _check(self, g):
        _check_sgd(g)
        if (g["momentum"] != 0) != (self.buf is not None):
            raise ValueError("SGD.load_state_dict: momentum == 0 and momentum != 0 are different kernels with different state; "
                             "build the optimizer with the momentum of the checkpoint")

    def _advance(self):
        self.t += 1
        self._first = not self._has_buf
        self._has_buf = True

    def _fill(self, h, g, ema_decay):
        first = self._first or self.buf is None
        h[0] = g["lr"]; h[1] = g["momentum"]
        h[2] = 0.0 if first else g["momentum"]
        h[3] = 1.0 if first else 1.0 - g["dampening"]
        h[4] = g["weight_decay"]; h[5] = float(bool(g["nesterov"])); h[6] = 0.0; h[7] = ema_decay

    def _kernel(self):
        return (0 if self.buf is None else 1), self.buf, None

    def _group(self, g):
        return dict(momentum=g["momentum"], dampening=g["dampening"], weight_decay=g["weight_decay"], nesterov=g["nesterov"],
                    maximize=False, foreach=None, differentiable=False, fused=None)

    def _state(self):
        """`torch.optim.SGD.state_dict()`: `momentum_buffer` per parameter once a step has run; nothing when momentum == 0."""
        if self.buf is None or not self._has_buf:
            return {}
        return self._per_param(momentum_buffer=self.buf)

    def _load(self, st):
        if st and self.buf is not None and st[0].get("momentum_buffer") is not None:
            self._flat(st, "momentum_buffer", self.buf)
            self._has_buf = True
        else:
            if self.buf is not None:
                self.buf.zero_()
            self._has_buf = False
        self._first = not self._has_buf


def get_optimizer(model, optim_name, lr):
    """`get_optimizer(model, optim_name, lr)` of main_train_masked.py:134-141 (`--optim {adam, adamw, sgd}`, :375): the name is
    case-insensitive, every other hyper-parameter is torch's default, and any other name fails as upstream's does (its
    `optimizer` is never bound)."""
    name = optim_name.lower()
    if name == "sgd":
        return SGD(model, lr=lr)
    if name == "adam":
        return Adam(model, lr=lr)
    if name == "adamw":
        return AdamW(model, lr=lr)
    raise UnboundLocalError(f"cannot access local variable 'optimizer' where it is not associated with a value (optim_name={optim_name!r})")


class EMA:
    """Flat-buffer EMA with diffusers' warm-up decay (see module docstring: not oracle-checked)."""

    def __init__(self, model, decay=0.9999, use_ema_warmup=True, inv_gamma=1.0, power=0.75, min_decay=0.0):
        self.model, self.pstore = model, model.store
        self.decay, self.use_ema_warmup, self.inv_gamma, self.power, self.min_decay = decay, use_ema_warmup, inv_gamma, power, min_decay
        self.shadow = model.store.P.clone()
        self.optimization_step = 0
        self._backup = None

    def get_decay(self, optimization_step):
        step = max(0, optimization_step - 1)
        if step <= 0:
            return 0.0
        if self.use_ema_warmup:
            v = 1 - (1 + step / self.inv_gamma) ** -self.power
        else:
            v = (1 + step) / (10 + step)
        return max(min(v, self.decay), self.min_decay)

    def next_decay(self):
        self.optimization_step += 1
        return self.get_decay(self.optimization_step)

    def step(self, parameters=None):
        d = self.next_decay()
        self.shadow.sub_((1 - d) * (self.shadow - self.pstore.P))

    def store(self, parameters=None):           # diffusers EMAModel.store / copy_to / restore
        self._backup = self.pstore.P.clone()

    def copy_to(self, parameters=None):
        self.pstore.P.copy_(self.shadow)
        self.pstore.sync_shadow()

    def restore(self, parameters=None):
        self.pstore.P.copy_(self._backup)
        self.pstore.sync_shadow()
        self._backup = None

    def state_dict(self):
        return dict(shadow=self.shadow, optimization_step=self.optimization_step)

    def config(self):
        """The fields diffusers' EMAModel.save_pretrained adds to the model config (main_train_masked.py:119-127, 200)."""
        return dict(decay=self.decay, min_decay=self.min_decay, optimization_step=self.optimization_step, update_after_step=0,
                    use_ema_warmup=self.use_ema_warmup, inv_gamma=self.inv_gamma, power=self.power)

    def load_reference(self, sd, cfg=None):
        """Shadow parameters from a {reference key: tensor} dict (+ the counters of `config()`)."""
        self.shadow.copy_(self.pstore.flat_from_reference(sd).to(self.shadow.device))
        if cfg:
            self.optimization_step = int(cfg.get("optimization_step", self.optimization_step))
            for k in ("decay", "min_decay", "use_ema_warmup", "inv_gamma", "power"):
                if k in cfg:
                    setattr(self, k, cfg[k])


class LambdaLR:
    def __init__(self, optimizer, fn):
        self.opt, self.fn, self.k = optimizer, fn, 0
        self.base = optimizer.param_groups[0]["initial_lr"]
        optimizer.param_groups[0]["lr"] = self.base * fn(0)

    def step(self):
        self.k += 1
        self.opt.param_groups[0]["lr"] = self.base * self.fn(self.k)

    def get_last_lr(self):
        return [self.opt.param_groups[0]["lr"]]

    def state_dict(self):          # torch.optim.lr_scheduler.LambdaLR.state_dict() fields (the lambda itself is not saved)
        return dict(base_lrs=[self.base], last_epoch=self.k, _step_count=self.k + 1, _is_initial=False, _get_lr_called_within_step=False,
                    _last_lr=self.get_last_lr(), lr_lambdas=[None])

    def load_state_dict(self, sd):
        self.k = int(sd["last_epoch"])
        self.base = sd["base_lrs"][0]
        self.opt.param_groups[0]["lr"] = self.base * self.fn(self.k)


def get_lr_scheduler(name, optimizer, num_warmup_steps, num_training_steps, num_cycles=0.5):
    """'cosine' | 'hard_cosine' | 'constant' | 'linear' with warm-up (main_train_masked.py:144-165)."""
    w = max(1, num_warmup_steps)

    def warm(k):
        return k / w if k < num_warmup_steps else None
    if name == "constant":
        return LambdaLR(optimizer, lambda k: warm(k) if warm(k) is not None else 1.0)
    if name == "linear":
        return LambdaLR(optimizer, lambda k: warm(k) if warm(k) is not None else
                        max(0.0, (num_training_steps - k) / max(1, num_training_steps - num_warmup_steps)))
    if name == "cosine":
        def f(k):
            if warm(k) is not None:
                return warm(k)
            p = (k - num_warmup_steps) / max(1, num_training_steps - num_warmup_steps)
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * num_cycles * 2.0 * p)))
        return LambdaLR(optimizer, f)
    if name == "hard_cosine":
        def f(k):
            if warm(k) is not None:
                return warm(k)
            p = (k - num_warmup_steps) / max(1, num_training_steps - num_warmup_steps)
            if p >= 1.0:
                return 0.0
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((num_cycles * p) % 1.0))))
        return LambdaLR(optimizer, f)
    raise ValueError(name)


class Accelerator:
    """The subset of `accelerate.Accelerator` the trainers touch, backed by
    torch.distributed (RCCL on ROCm) when a process group is initialised."""

    def __init__(self, gradient_accumulation_steps=1, mixed_precision="bf16", device=None, split_batches=False):
        import torch.distributed as dist
        self.dist = dist if dist.is_available() and dist.is_initialized() else None
        self.num_processes = self.dist.get_world_size() if self.dist else 1
        self.process_index = self.dist.get_rank() if self.dist else 0
        self.mixed_precision = mixed_precision
        self.gradient_accumulation_steps = int(gradient_accumulation_steps)
        if self.gradient_accumulation_steps < 1:
            raise ValueError(f"gradient_accumulation_steps={gradient_accumulation_steps}")
        self.split_batches = split_batches       # accelerate default False: the LR schedule then steps num_processes times per update
        self.sync_gradients = True
        self.end_of_dataloader = False           # set by the trainer's batch loop (accelerate: by its prepared dataloader)
        self.step = 0
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
        self._ckpt = {}

    @property
    def is_main_process(self):
        return self.process_index == 0

    is_local_main_process = is_main_process

    def prepare(self, *objs):
        from .data import DeviceLoader
        from .unet import UNet
        for o in objs:                      # main_train_masked.py:299-307: model, optimizer, dataloader, lr_scheduler
            if isinstance(o, DeviceLoader):          # this rank's batches of the common order; every other loader is returned as it is
                o.rank, o.world = self.process_index, self.num_processes
            elif isinstance(o, UNet):
                self._ckpt["model"] = o
            elif isinstance(o, _FlatOptimizer):      # AdamW | Adam | SGD
                self._ckpt["optimizer"] = o
            elif isinstance(o, LambdaLR):
                self._ckpt["lr_scheduler"] = o
            elif isinstance(o, EMA):
                self._ckpt["ema"] = o
        return objs if len(objs) != 1 else objs[0]

    def accumulate(self, model=None):
        """`with accelerator.accumulate(model):` (ms:139) -- accelerate's `_do_sync`: the micro-step counter decides
        `sync_gradients`; the last batch of the dataloader always syncs and restarts the count.  What upstream hangs on the
        flag (scaled backward, clip, optimizer / LR step, EMA) is done by TrainStep / Trainer._step."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            if self.end_of_dataloader:
                self.step = 0
                self.sync_gradients = True
            else:
                self.step += 1
                self.sync_gradients = (self.step % self.gradient_accumulation_steps) == 0
            yield
        return ctx()

    def backward(self, loss):       # the fused train step has already produced the gradients
        return None

    def clip_grad_norm_(self, params, max_norm):
        return None

    def wait_for_everyone(self):
        if self.dist:
            self.dist.barrier()

    def print(self, *a, **k):
        if self.is_main_process:
            print(*a, **k)

    def register_for_checkpointing(self, **objs):
        """model=, optimizer=, ema=, lr_scheduler=, scheduler= : what `save_state(path)` / `load_state(path)` cover.
        (`prepare()` registers what it recognises; the trainers register the rest.)"""
        for k, v in objs.items():
            if v is not None:
                self._ckpt[k] = v

    def save_state(self, output_dir=None, model=None, optimizer=None, ema=None, **extra):
        """`accelerator.save_state(path)` (trainer_masked_mean_shift.py:267-268) in the reference's directory
        layout (mdm/checkpoint.py).  Called with the path alone, like upstream, it saves the registered objects."""
        from . import checkpoint
        c = dict(self._ckpt)
        c.update({k: v for k, v in dict(model=model, optimizer=optimizer, ema=ema).items() if v is not None})
        if c.get("model") is None:
            raise RuntimeError("Accelerator.save_state: no model registered (prepare() / register_for_checkpointing())")
        checkpoint.save_state(output_dir, c["model"], c.get("optimizer"), c.get("ema"), c.get("lr_scheduler"), c.get("scheduler"),
                              rank=self.process_index, main=self.is_main_process, extra=extra or None, step=self.step)
        self.wait_for_everyone()
        return output_dir

    def load_state(self, input_dir=None):
        """`accelerator.load_state(path)` (main_train_masked.py:268): restores every registered object in place."""
        from . import checkpoint
        c = self._ckpt
        if c.get("model") is None:
            raise RuntimeError("Accelerator.load_state: no model registered (prepare() / register_for_checkpointing())")
        extra = checkpoint.load_state(input_dir, c["model"], c.get("optimizer"), c.get("ema"), c.get("lr_scheduler"), c.get("scheduler"),
                                      rank=self.process_index)
        self.step = int(extra.get("step", self.step))          # accelerate restores its micro-step counter too
        return extra
