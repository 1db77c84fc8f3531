"""ctypes binding of libmdm_hip.so.

include/mdm_hip.h is the only statement of the C ABI: the two descriptor structs, every prototype and the parameter
names below are parsed from it at import.  To add an entry point, declare it in the header -- nothing else.
include/mdm_vis.h is the presentation ABI of the same library (image grids, `mdm_vis_*`): parsed the same way into
`VIS_PROTOS` / `VIS_EXPORTS`, bound by `load()` and served by `call` and `Recording` next to the core table.
include/mdm_data.h is the data ABI (the device-resident data set, `mdm_data_*`): `DATA_PROTOS` / `DATA_EXPORTS`, the same way.
include/mdm_interp.h is the interpolation-sampler ABI (`mdm_interp_*`): `INTERP_PROTOS` / `INTERP_EXPORTS`, the same way.
include/mdm_ingest.h is the ingest ABI (image files into the device data set, `mdm_ingest_*`): `INGEST_PROTOS` / `INGEST_EXPORTS`.
include/mdm_neighbor.h is the nearest-neighbour ABI (feature rows of the stored set, `mdm_nn_*`): `NEIGHBOR_PROTOS` / `NEIGHBOR_EXPORTS`.
include/mdm_inpaint.h is the inpainting-sampler ABI (`mdm_inpaint_*`): `INPAINT_PROTOS` / `INPAINT_EXPORTS`.
include/mdm_metric.h is the image-quality ABI (MSE, PSNR, SSIM, `mdm_metric_*`): `METRIC_PROTOS` / `METRIC_EXPORTS`.
include/mdm_restore.h is the restoration-sampler ABI (group-mean projection, `mdm_restore_*`): `RESTORE_PROTOS` / `RESTORE_EXPORTS`.
include/mdm_moment.h is the set-moment ABI (fp64 first and second moments of feature rows, `mdm_moment_*`): `MOMENT_PROTOS` / `MOMENT_EXPORTS`.

The product path has NO fallback: if the shared library or the header is missing, or a call
returns non-zero, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect
import os
import re

import torch

F32, BF16 = 0, 1
_HERE = os.path.dirname(os.path.abspath(__file__))
# (MDM_LIB_PATH: load another BUILD of the same library -- A/B timing of two builds on one box; it selects a file, not a code path)
LIB_PATH = os.environ.get("MDM_LIB_PATH") or os.path.join(_HERE, "libmdm_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "mdm_hip.h"))
VIS_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "mdm_vis.h")
DATA_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "mdm_data.h")
INTERP_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "mdm_interp.h")
INGEST_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "mdm_ingest.h")
NEIGHBOR_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "mdm_neighbor.h")
INPAINT_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "mdm_inpaint.h")
METRIC_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "mdm_metric.h")
RESTORE_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "mdm_restore.h")
MOMENT_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "mdm_moment.h")

vp, i32, i64, u64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float
_SCALARS = {"int": i32, "int32_t": i32, "int64_t": i64, "uint64_t": u64, "float": f32}

_TOP = re.compile(r'\s*(?:extern\s+"C"\s*\{|\}|typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;|([^;{}()]+)\(([^;{}()]*)\)\s*;)')
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*(\**)\s*(\w*)\s*(\[\d+\])?")


def _declaration(text, where, param=False):
    """`[const] T[*..] name` -> (name, type): type "T" for a known scalar, "T*" / "T**" for any pointer; a parameter `T name[n]`
    is the pointer C makes of it.  Everything else raises."""
    m = _DECL.fullmatch(text.strip())
    if not m or (m.group(4) and not param):
        raise ValueError(f"mdm_hip.h: cannot split `{text.strip()}` into type and name in `{where}`")
    base, stars, name = m.group(1), m.group(2) + ("*" if m.group(4) else ""), m.group(3)
    if not name:
        raise ValueError(f"mdm_hip.h: `{text.strip()}` has no name in `{where}`")
    if not stars and base not in _SCALARS:
        raise ValueError(f"mdm_hip.h: unknown type `{base}` of `{name}` in `{where}`")
    return name, base + stars


def parse_header(text):
    """The C ABI as text -> ({struct: [(field, type)]}, {function: (return type, [(parameter, type)])}) in the header's order.
    Closed: whatever is not a comment, a preprocessor line, the `extern "C"` bracket, a `typedef struct` or a prototype raises,
    and so does every declaration `_declaration` refuses.  Nothing is skipped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs, protos, pos = {}, {}, 0
    while text[pos:].strip():
        m = _TOP.match(text, pos)
        if not m:
            raise ValueError(f"mdm_hip.h: cannot parse `{' '.join(text[pos:].split())[:80]}`")
        pos, where = m.end(), " ".join(m.group(0).split())
        body, struct, head, params = m.groups()
        if struct:
            fields = structs[struct] = []
            for stmt in filter(None, (s.strip() for s in body.split(";"))):
                first, *more = stmt.split(",")
                name, typ = _declaration(first, f"{struct}: {stmt}")
                if more and typ not in _SCALARS:      # `float* a, b` declares ONE pointer
                    raise ValueError(f"mdm_hip.h: one pointer per declaration in `{struct}: {stmt}`")
                fields += [(name, typ)] + [_declaration(f"{typ} {n}", f"{struct}: {stmt}") for n in more]
        elif head:
            name, rtype = _declaration(head, where)
            protos[name] = (rtype, [] if params.strip() in ("", "void") else [_declaration(p, where, param=True) for p in params.split(",")])
    return structs, protos


def _read_headers(core, extra):
    """Parse the core header, then every `(path, prefix)` of `extra`: such a header declares functions named `prefix*` only -- no
    struct, no name that a header before it declares.  -> (core structs, core prototypes, [prototypes of each extra header])."""
    parsed = []
    for path, prefix in ((core, None), *extra):
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: it is the only statement of libmdm_hip.so's C ABI and this binding is built from it at import "
                "(include/ sits next to masked-diffusion-model_amd/).  There is no fallback.")
        with open(path) as f:
            structs, decls = parse_header(f.read())
        seen = set().union(*(d for _, d in parsed))
        if prefix is not None and (structs or set(decls) & seen or not all(n.startswith(prefix) for n in decls)):
            raise RuntimeError(f"{path}: this header declares `{prefix}*` functions only, none of them twice")
        parsed.append((structs, decls))
    return parsed[0][0], parsed[0][1], [d for _, d in parsed[1:]]


_STRUCTS, _DECLS, (_VIS_DECLS, _DATA_DECLS, _INTERP_DECLS, _INGEST_DECLS, _NEIGHBOR_DECLS, _INPAINT_DECLS,
                    _METRIC_DECLS, _RESTORE_DECLS, _MOMENT_DECLS) = _read_headers(
    HEADER_PATH, ((VIS_HEADER_PATH, "mdm_vis_"), (DATA_HEADER_PATH, "mdm_data_"), (INTERP_HEADER_PATH, "mdm_interp_"),
                  (INGEST_HEADER_PATH, "mdm_ingest_"), (NEIGHBOR_HEADER_PATH, "mdm_nn_"), (INPAINT_HEADER_PATH, "mdm_inpaint_"),
                  (METRIC_HEADER_PATH, "mdm_metric_"), (RESTORE_HEADER_PATH, "mdm_restore_"),
                  (MOMENT_HEADER_PATH, "mdm_moment_")))

_DESC_PTR = {}


def _ctype(typ, ret=False):
    """Scalars by name; a pointer to a descriptor struct is typed; a returned `const char*` is bytes; every other pointer is void*."""
    return C.c_char_p if ret and typ == "char*" else _SCALARS.get(typ) or _DESC_PTR.get(typ, vp)


class GemmDesc(C.Structure):
    """`mdm_gemm_desc` as include/mdm_hip.h declares it: the header is the only statement, a new field goes there and nowhere else."""
    _fields_ = [(n, _ctype(t)) for n, t in _STRUCTS["mdm_gemm_desc"]]
    _defaults = dict(alpha=1.0, batch=1)


class GnDesc(C.Structure):
    """`mdm_gn_desc` as include/mdm_hip.h declares it: the header is the only statement, a new field goes there and nowhere else."""
    _fields_ = [(n, _ctype(t)) for n, t in _STRUCTS["mdm_gn_desc"]]
    _defaults = {}


_DESC_PTR.update({"mdm_gemm_desc*": C.POINTER(GemmDesc), "mdm_gn_desc*": C.POINTER(GnDesc)})
def _tables(decls):
    """{name: (argtypes, restype)}, {name: parameter names} and the names, in the header's order."""
    protos = {name: ([_ctype(t) for _, t in params], _ctype(rtype, ret=True)) for name, (rtype, params) in decls.items()}
    return protos, {name: [n for n, _ in params] for name, (_, params) in decls.items()}, list(protos)


# every function the core header declares ...
_PROTOS, _PARAMS, EXPORTS = _tables(_DECLS)
# ... and the same three tables of include/mdm_vis.h, mdm_data.h, mdm_interp.h, mdm_ingest.h, mdm_neighbor.h, mdm_inpaint.h, mdm_metric.h, mdm_restore.h and mdm_moment.h, kept apart: the core tables are exactly what
# mdm_hip.h declares
VIS_PROTOS, VIS_PARAMS, VIS_EXPORTS = _tables(_VIS_DECLS)
DATA_PROTOS, DATA_PARAMS, DATA_EXPORTS = _tables(_DATA_DECLS)
INTERP_PROTOS, INTERP_PARAMS, INTERP_EXPORTS = _tables(_INTERP_DECLS)
INGEST_PROTOS, INGEST_PARAMS, INGEST_EXPORTS = _tables(_INGEST_DECLS)
NEIGHBOR_PROTOS, NEIGHBOR_PARAMS, NEIGHBOR_EXPORTS = _tables(_NEIGHBOR_DECLS)
INPAINT_PROTOS, INPAINT_PARAMS, INPAINT_EXPORTS = _tables(_INPAINT_DECLS)
METRIC_PROTOS, METRIC_PARAMS, METRIC_EXPORTS = _tables(_METRIC_DECLS)
RESTORE_PROTOS, RESTORE_PARAMS, RESTORE_EXPORTS = _tables(_RESTORE_DECLS)
MOMENT_PROTOS, MOMENT_PARAMS, MOMENT_EXPORTS = _tables(_MOMENT_DECLS)
_ALL_PROTOS = {**_PROTOS, **VIS_PROTOS, **DATA_PROTOS, **INTERP_PROTOS, **INGEST_PROTOS, **NEIGHBOR_PROTOS, **INPAINT_PROTOS, **METRIC_PROTOS,
               **RESTORE_PROTOS, **MOMENT_PROTOS}
_ALL_PARAMS = {**_PARAMS, **VIS_PARAMS, **DATA_PARAMS, **INTERP_PARAMS, **INGEST_PARAMS, **NEIGHBOR_PARAMS, **INPAINT_PARAMS, **METRIC_PARAMS,
               **RESTORE_PARAMS, **MOMENT_PARAMS}

_lib = None


def load():
    """Load the library once; raise loudly if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C masked-diffusion-model_amd/csrc`).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (args, res) in _ALL_PROTOS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().mdm_last_error().decode()
        raise RuntimeError(f"libmdm_hip {what} failed ({rc}): {msg}")


class Recording:
    """A recorded launch sequence: every C-ABI call made while it is active is appended
    (function, args-without-stream) instead of being executed; `run()` replays the list on
    the current stream.  All kernel entry points take the stream as their LAST argument."""

    def __init__(self):
        self.calls = []
        self.keep = []      # objects (descriptors, tensors) that must outlive the list
        self.flops = {}     # call index -> (algorithmic FLOPs, dtype) for contraction launches

    def __enter__(self):
        global _recording
        self._prev = _recording
        _recording = self
        return self

    def __exit__(self, *exc):
        global _recording
        _recording = self._prev
        return False

    def run(self, st=None):
        st = stream() if st is None else st
        for name, fn, args in self.calls:
            rc = fn(*args, st)
            if rc != 0:
                check(rc, name)

    def extend(self, other):
        base = len(self.calls)
        self.calls.extend(other.calls)
        self.keep.extend(other.keep)
        for i, v in other.flops.items():
            self.flops[base + i] = v

    def run_timed(self, st, pick, overhead_ms=0.0):
        """Replay eagerly with a HIP event pair around every launch `pick(index, name)` selects;
        returns [(index, ms)] (events sit on the launch stream `st`; `overhead_ms`, see
        `event_overhead`, is taken off every reading)."""
        lib = load()
        pairs = []
        for i, (name, fn, args) in enumerate(self.calls):
            if pick(i, name):
                a, b = vp(), vp()
                check(lib.mdm_event_create(C.byref(a))); check(lib.mdm_event_create(C.byref(b)))
                check(lib.mdm_event_record(a, st))
                check(fn(*args, st), name)
                check(lib.mdm_event_record(b, st))
                pairs.append((i, a, b))
            else:
                check(fn(*args, st), name)
        out = []
        for i, a, b in pairs:
            ms = f32()
            check(lib.mdm_event_elapsed_ms(a, b, C.byref(ms)))
            out.append((i, max(ms.value - overhead_ms, 0.0)))
            lib.mdm_event_destroy(a); lib.mdm_event_destroy(b)
        return out

    def event_overhead(self, st, pick, n=24):
        """What an event pair adds to the launch it brackets: for the first `n` picked calls (they must be
        idempotent: forward contractions) compare a pair around ONE launch with a pair around TWO back-to-back
        launches; overhead = 2 T1 - T2.  Median over the sample, in ms."""
        lib = load()
        def timed(fn, args, reps):
            a, b = vp(), vp()
            check(lib.mdm_event_create(C.byref(a))); check(lib.mdm_event_create(C.byref(b)))
            check(lib.mdm_event_record(a, st))
            for _ in range(reps):
                check(fn(*args, st))
            check(lib.mdm_event_record(b, st))
            check(lib.mdm_stream_sync(st))
            ms = f32()
            check(lib.mdm_event_elapsed_ms(a, b, C.byref(ms)))
            lib.mdm_event_destroy(a); lib.mdm_event_destroy(b)
            return ms.value
        est = []
        for i, (name, fn, args) in enumerate(self.calls):
            if len(est) >= n:
                break
            if name == "mdm_gemm" and pick(i, name):
                timed(fn, args, 1)                      # warm
                t1 = min(timed(fn, args, 1) for _ in range(3))
                t2 = min(timed(fn, args, 2) for _ in range(3))
                est.append(2.0 * t1 - t2)
        est.sort()
        return max(est[len(est) // 2], 0.0) if est else 0.0


_recording = None


class GraphExec:
    """A hipGraph instantiated from a Recording (captured on a private stream, replayed on the
    caller's current stream)."""

    def __init__(self, rec):
        self.rec = rec                      # keeps descriptors/tensors alive
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        handle = vp()
        with torch.cuda.stream(side):
            check(load().mdm_graph_begin(side.cuda_stream), "mdm_graph_begin")
            try:
                rec.run(side.cuda_stream)
            finally:
                rc = load().mdm_graph_end(side.cuda_stream, C.byref(handle))
            check(rc, "mdm_graph_end")
        cur.wait_stream(side)
        self.handle = handle

    def launch(self, st=None):
        check(load().mdm_graph_launch(self.handle, stream() if st is None else st), "mdm_graph_launch")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                load().mdm_graph_destroy(self.handle)
        except Exception:
            pass


@functools.lru_cache(maxsize=None)
def _signature(name):
    return inspect.Signature([inspect.Parameter(p, inspect.Parameter.POSITIONAL_OR_KEYWORD) for p in _ALL_PARAMS[name]])


def call(name, *args, **kw):
    """Call a kernel entry point (last parameter = stream) or record it.  Keywords are the header's parameter names; they are
    bound into the positional tuple first, so a wrong, missing or doubled name is a TypeError before anything is launched or
    recorded.  Nothing is defaulted."""
    fn = getattr(load(), name)
    if kw:
        try:
            args = _signature(name).bind(*args, **kw).args
        except TypeError as e:
            raise TypeError(f"{name}: {e}") from None
    if _recording is not None:
        _recording.calls.append((name, fn, args[:-1]))
        _recording.keep.append(args)
        return
    check(fn(*args), name)


def ptr(t):
    """Device pointer of a tensor (or None)."""
    if t is None:
        return None
    return t.data_ptr()


def stream():
    """The HIP stream kernels are launched on: torch's current stream of the current device."""
    if _recording is not None:
        return None        # filled in at replay time
    if not torch.cuda.is_available():
        return None        # no device: argument checks still run, any launch then fails loudly in HIP
    return torch.cuda.current_stream().cuda_stream


def torch_dtype(dt):
    return torch.float32 if dt == F32 else torch.bfloat16


def _desc(kw, cls=GemmDesc):
    """A `cls` descriptor from keyword fields: tensors become device pointers, None a null pointer, the rest stays zero."""
    d = cls(**cls._defaults)
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            v = v.data_ptr()
        setattr(d, k, v)
    return d


def gemm_plan(**kw):
    """(split count, workspace bytes) mdm_gemm would use for these fields given unlimited workspace; no launch."""
    kw.pop("_flops", None)
    d = _desc(kw)
    sk, nb = i32(), i64()
    check(load().mdm_gemm_plan(C.byref(d), C.byref(sk), C.byref(nb)), "mdm_gemm_plan")
    return sk.value, nb.value


def _desc_array(fields_list):
    arr = (GemmDesc * len(fields_list))()
    for i, f in enumerate(fields_list):
        d = _desc({k: v for k, v in f.items() if k != "_flops"})
        C.memmove(C.byref(arr, i * C.sizeof(GemmDesc)), C.byref(d), C.sizeof(GemmDesc))
    return arr


def wgrad_group_schedule(fields_list, n_cu):
    """The table WgradGroup(fields_list) would upload on a device of `n_cu` CUs, decoded (mdm_wgrad_group_schedule, no device):
    -> (rows, need_bytes, form): one tuple (queue, round, desc, kind, tile_or_item, k0, k1, slot) per table entry, padding
    included; the bytes of the device table; 0 = per-tap flat grid, 1 = merged persistent launch."""
    lib, arr, n = load(), _desc_array(fields_list), len(fields_list)
    n_rows, need, form = i64(), i64(), i32()
    check(lib.mdm_wgrad_group_schedule(arr, n, n_cu, None, 0, C.byref(n_rows), C.byref(need), C.byref(form)), "mdm_wgrad_group_schedule")
    rows = (i32 * (8 * n_rows.value))()
    check(lib.mdm_wgrad_group_schedule(arr, n, n_cu, rows, n_rows.value, C.byref(n_rows), C.byref(need), C.byref(form)),
          "mdm_wgrad_group_schedule")
    flat = list(rows)
    return [tuple(flat[i:i + 8]) for i in range(0, len(flat), 8)], need.value, form.value


class WgradGroup:
    """Handle of mdm_wgrad_group_*: a set of weight-gradient descriptors that run as ONE launch (+ one launch summing
    their split-K partials).  `fields_list`: keyword dicts like `gemm()` takes.  The device table lives in a tensor
    owned here; operands are referenced by pointer, so the caller keeps them alive."""

    def __init__(self, fields_list, device):
        lib = load()
        n = len(fields_list)
        self.flops = sum(f.pop("_flops", 0.0) for f in fields_list)
        arr = _desc_array(fields_list)
        need, h = i64(), vp()
        check(lib.mdm_wgrad_group_create(arr, n, None, 0, C.byref(need), C.byref(h)), "mdm_wgrad_group_create")
        self.table = torch.empty(need.value, dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)
        check(lib.mdm_wgrad_group_create(arr, n, self.table.data_ptr(), need.value, C.byref(need), C.byref(h)), "mdm_wgrad_group_create")
        assert h.value, "wgrad group was not built"
        self.handle, self.n, self.keep = h, n, fields_list

    def launch(self):
        """Launch (or record) the group on the current stream."""
        if _recording is not None:
            _recording.keep.append(self)
            _recording.flops[len(_recording.calls)] = (self.flops, BF16)
        call("mdm_wgrad_group_launch", self.handle, stream())

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                load().mdm_wgrad_group_destroy(self.handle)
        except Exception:
            pass


def last_route():
    """Kernel (and second stage) of the last mdm_gemm / mdm_gemm_pair / wgrad group launch on this thread (mdm_gemm_last_route)."""
    return load().mdm_gemm_last_route().decode()


def route_of(**kw):
    """What last_route() would name after gemm(**kw), without launching (mdm_gemm_route_of); "none" for a refused descriptor."""
    kw.pop("_flops", None)
    return load().mdm_gemm_route_of(C.byref(_desc(kw))).decode()


def pair_route_of(kw_a, kw_b):
    """What last_route() would name after gemm_pair(kw_a, kw_b), without launching (mdm_gemm_pair_route_of)."""
    da, db = (_desc({k: v for k, v in kw.items() if k != "_flops"}) for kw in (kw_a, kw_b))
    return load().mdm_gemm_pair_route_of(C.byref(da), C.byref(db)).decode()


def launch_of(**kw):
    """The first launch gemm(**kw) would make, without making it (mdm_gemm_launch_of): (workgroups, grid z, threads per workgroup,
    dynamic LDS bytes, tile rows, tile columns), or None for a refused descriptor."""
    kw.pop("_flops", None)
    out = (i32 * 6)()
    return tuple(out) if load().mdm_gemm_launch_of(C.byref(_desc(kw)), out) == 0 else None


def pair_launch_of(kw_a, kw_b):
    """The fused launch of gemm_pair(kw_a, kw_b) like launch_of (mdm_gemm_pair_launch_of); the two launch_of tuples where the pair
    runs as two launches; None for a refused pair."""
    da, db = (_desc({k: v for k, v in kw.items() if k != "_flops"}) for kw in (kw_a, kw_b))
    out = (i32 * 6)()
    rc = load().mdm_gemm_pair_launch_of(C.byref(da), C.byref(db), out)
    return tuple(out) if rc == 0 else (launch_of(**kw_a), launch_of(**kw_b)) if rc == 1 else None


def wgrad_split_last_route():
    """Kernel (and second stage) of the last mdm_conv_wgrad_split call on this thread (mdm_wgrad_split_last_route)."""
    return load().mdm_wgrad_split_last_route().decode()


def wgrad_split(**kw):
    """The weight-gradient fields of a descriptor through mdm_conv_wgrad_split (split products): launch / record it."""
    flops = kw.pop("_flops", None)
    d = _desc(kw)
    if _recording is not None:
        _recording.keep.append((d, kw))
        _recording.flops[len(_recording.calls)] = (flops if flops is not None else 2.0 * d.M * d.N * d.K, d.dtype)
    call("mdm_conv_wgrad_split", C.byref(d), stream())
    return d


def wgrad_split_plan(**kw):
    """(split count, workspace bytes) mdm_conv_wgrad_split would use for these fields; no launch."""
    kw.pop("_flops", None)
    d = _desc(kw)
    sk, nb = i32(), i64()
    check(load().mdm_conv_wgrad_split_plan(C.byref(d), C.byref(sk), C.byref(nb)), "mdm_conv_wgrad_split_plan")
    return sk.value, nb.value


def note(fn):
    """Run the host callable `fn()` at this point of the launch sequence: at once, or -- inside a Recording -- every time the
    recording is replayed or captured (host code only, nothing is enqueued)."""
    if _recording is not None:
        _recording.calls.append(("note", lambda st: (fn(), 0)[1], ()))
        return
    fn()


def route_names():
    """Every name last_route() can return."""
    lib = load()
    n = lib.mdm_gemm_route_names(None, 0)
    arr = (C.c_char_p * n)()
    lib.mdm_gemm_route_names(arr, n)
    return [v.decode() for v in arr]


def attn_route_of(which, dt, L, C):
    """The fused attention kernel mdm_attn_fwd (which = 0) / mdm_attn_bwd (1) would launch, e.g. "fwd_dma<256>", without
    launching (mdm_attn_route_of); None for a request they refuse."""
    r = load().mdm_attn_route_of(which, dt, L, C)
    return None if r is None else r.decode()


def attn_last_route():
    """Kernel of the last mdm_attn_fwd / mdm_attn_bwd call on this thread (mdm_attn_last_route); "none" after a refused one."""
    return load().mdm_attn_last_route().decode()


def attn_route_names():
    """Every name attn_route_of() / attn_last_route() can return."""
    lib = load()
    n = lib.mdm_attn_route_names(None, 0)
    arr = (C.c_char_p * n)()
    lib.mdm_attn_route_names(arr, n)
    return [v.decode() for v in arr]


def gn_route_of(which, **fields):
    """The GroupNorm kernel mdm_groupnorm_fwd (which = 0) / mdm_groupnorm_bwd (1) would launch for a descriptor with these
    fields, e.g. "fwd_reg<4,512>", without launching (mdm_gn_route_of); None for a shape or dtype they refuse."""
    r = load().mdm_gn_route_of(which, C.byref(_desc(fields, GnDesc)))
    return None if r is None else r.decode()


def gn_last_route():
    """Kernel of the last mdm_groupnorm_fwd / mdm_groupnorm_bwd call on this thread (mdm_gn_last_route); "none" after a refused one."""
    return load().mdm_gn_last_route().decode()


def gn_route_names():
    """Every name gn_route_of() / gn_last_route() can return."""
    lib = load()
    n = lib.mdm_gn_route_names(None, 0)
    arr = (C.c_char_p * n)()
    lib.mdm_gn_route_names(arr, n)
    return [v.decode() for v in arr]


def skinny_route_of(which, M, N, K, has_t=False):
    """The kernel mdm_skinny_linear_fwd (which = 0) / mdm_skinny_linear_bwd (1) would launch, e.g. "nt<2,1,temb>", without
    launching (mdm_skinny_route_of); None for a shape they refuse."""
    r = load().mdm_skinny_route_of(which, M, N, K, int(bool(has_t)))
    return None if r is None else r.decode()


def skinny_last_route():
    """Kernel of the last mdm_skinny_linear_fwd / _bwd call on this thread (mdm_skinny_last_route); "none" after a refused one."""
    return load().mdm_skinny_last_route().decode()


def skinny_route_names():
    """Every name skinny_route_of() / skinny_last_route() can return."""
    lib = load()
    n = lib.mdm_skinny_route_names(None, 0)
    arr = (C.c_char_p * n)()
    lib.mdm_skinny_route_names(arr, n)
    return [v.decode() for v in arr]


def wgrad_group_accepts(**kw):
    kw.pop("_flops", None)
    return bool(load().mdm_wgrad_group_accepts(C.byref(_desc(kw))))


def gemm_pair(kw_a, kw_b):
    """Two independent contractions as ONE call (mdm_gemm_pair): -> (desc_a, desc_b)."""
    fa, fb = kw_a.pop("_flops", None), kw_b.pop("_flops", None)
    da, db = _desc(kw_a), _desc(kw_b)
    if _recording is not None:
        _recording.keep.append((da, kw_a, db, kw_b))
        fl = lambda f, d: f if f is not None else 2.0 * d.M * d.N * d.K * d.batch
        _recording.flops[len(_recording.calls)] = (fl(fa, da) + fl(fb, db), da.dtype)
    call("mdm_gemm_pair", C.byref(da), C.byref(db), stream())
    return da, db


def gemm(**kw):
    """Fill a descriptor from keyword fields (tensors become device pointers) and launch / record it."""
    flops = kw.pop("_flops", None)
    d = _desc(kw)
    if _recording is not None:
        _recording.keep.append((d, kw))
        # algorithmic FLOPs of this launch, keyed by its index in the recording (bench.py roofline)
        _recording.flops[len(_recording.calls)] = (flops if flops is not None else 2.0 * d.M * d.N * d.K * d.batch, d.dtype)
    call("mdm_gemm", C.byref(d), stream())
    return d


def groupnorm(name, **kw):
    """Fill a `GnDesc` from keyword fields like `gemm()` and launch / record `name` (mdm_groupnorm_fwd | mdm_groupnorm_bwd)."""
    d = _desc(kw, GnDesc)
    if _recording is not None:
        _recording.keep.append((d, kw))
    call(name, C.byref(d), stream())
    return d
