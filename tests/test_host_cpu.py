"""CPU-only tests: the C-ABI library loads and exports every symbol of include/mdm_hip.h, the
host-side logic (schedule tables, parameter layout, state_dict grammar, bucket planning, EMA/LR
schedules) and the data-parallel exchange over gloo with 2 processes.  No kernel is launched."""
import ctypes
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from golden.make_golden import TINY, base_args  # noqa: E402


# ------------------------------------------------------------------------------- C ABI
def test_library_exports_every_declared_symbol():
    from mdm import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    declared = set(re.findall(r"\b(mdm_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 30
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in mdm_hip.h but not exported"
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert lib.mdm_version() == 1


def test_descriptor_layout_matches_the_header(tmp_path):
    """Both descriptors completely: sizeof, then offset and size of EVERY field of GemmDesc and GnDesc against the header as a C
    compiler lays it out.  The field list comes from the class and must equal the struct's declarators as a regex of this test
    counts them (every identifier in front of a `,` or `;`), so a parser that drops or invents a member fails.  mdm_gn_desc has
    no implicit padding: its field sizes add up to sizeof.  (mdm_gemm_desc has 8 bytes of it by design.)"""
    from mdm._lib import GemmDesc, GnDesc
    hdr = os.path.join(ROOT, "include", "mdm_hip.h")
    text = re.sub(r"/\*.*?\*/", " ", open(hdr).read(), flags=re.S)
    structs = {"mdm_gemm_desc": GemmDesc, "mdm_gn_desc": GnDesc}
    prints = []
    for cname, cls in structs.items():
        fields = [name for name, _ in cls._fields_]
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (cname, cname), text, flags=re.S).group(1)
        assert fields == re.findall(r"(\w+)\s*[,;]", body), cname
        prints.append('printf("%%zu\\n",sizeof(%s));\n' % cname)
        prints += ['printf("%s %%zu %%zu\\n",offsetof(%s,%s),sizeof(((%s*)0)->%s));\n' % (f, cname, f, cname, f) for f in fields]
    assert (len(GemmDesc._fields_), len(GnDesc._fields_)) == (78, 30)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){%sreturn 0;}\n' % (hdr, "".join(prints)))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    lines = iter(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, cls in structs.items():
        size = int(next(lines))
        assert size == ctypes.sizeof(cls), cname
        c_fields = [(ln.split()[0], int(ln.split()[1]), int(ln.split()[2])) for ln in (next(lines) for _ in cls._fields_)]
        assert c_fields == [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_], cname
        if cls is GnDesc:
            assert sum(sz for _, _, sz in c_fields) == size == sum(getattr(cls, f).size for f, _ in cls._fields_)
    assert ctypes.sizeof(GemmDesc) == 448 and next(lines, None) is None


PARSER_REFUSALS = [      # header text, what the message must name
    ("int mdm_x(int n, unsigned flags, void* stream);", ("unknown type", "unsigned", "mdm_x")),
    ("typedef struct mdm_s { int32_t a; double b; } mdm_s;", ("unknown type", "double", "mdm_s")),
    ("int mdm_x(int n, const float*, void* stream);", ("no name", "const float*", "mdm_x")),
    ("int mdm_x(int, void* stream);", ("no name", "mdm_x")),
    ("int mdm_x(unsigned int n, void* stream);", ("cannot split", "unsigned int n", "mdm_x")),
    ("typedef struct mdm_s { float* a, b; } mdm_s;", ("one pointer per declaration", "mdm_s")),
    ("int mdm_x(int n, void* stream);\nstruct mdm_t;\n", ("cannot parse", "struct mdm_t")),
    ("typedef struct mdm_s { int32_t a[4]; } mdm_s;", ("cannot split", "a[4]", "mdm_s")),      # an array is a pointer in a parameter only
]


@pytest.mark.parametrize("text,named", PARSER_REFUSALS, ids=[" ".join(n[:2]) for _, n in PARSER_REFUSALS])
def test_header_parser_refuses_what_it_does_not_know(text, named):
    """The parser is closed: an unknown type, a declaration without a name or one it cannot split, and a construct that is neither
    a struct nor a prototype raise and name the declaration; nothing is skipped."""
    from mdm import _lib
    with pytest.raises(ValueError) as e:
        _lib.parse_header(text)
    for word in named:
        assert word in str(e.value), (word, str(e.value))


def test_header_parser_reads_a_prototype_over_three_lines():
    from mdm import _lib
    structs, protos = _lib.parse_header(
        "#define X 1\ntypedef struct mdm_s { const void* p; int32_t a, b; /* two */ float c; } mdm_s;\n"
        "int64_t mdm_x(const mdm_s* d_host, int n,   /* rows; cols, (both) */\n"
        "              const uint64_t* rng,\n"
        "              float scale, void* stream);\nconst char* mdm_y(void);\n")
    assert structs == {"mdm_s": [("p", "void*"), ("a", "int32_t"), ("b", "int32_t"), ("c", "float")]}
    assert protos == {"mdm_x": ("int64_t", [("d_host", "mdm_s*"), ("n", "int"), ("rng", "uint64_t*"), ("scale", "float"), ("stream", "void*")]),
                      "mdm_y": ("char*", [])}


def test_a_missing_header_is_a_loud_error(tmp_path):
    """The binding is built from the header at import: without it there is a RuntimeError that says so, not a partial module."""
    pkg = tmp_path / "masked-diffusion-model_amd" / "mdm"
    pkg.mkdir(parents=True)
    import mdm._lib as real
    (pkg / "_lib.py").write_text(open(real.__file__).read())
    (pkg / "__init__.py").write_text("")
    r = subprocess.run([sys.executable, "-c", "import mdm._lib"], cwd=str(pkg.parent), capture_output=True, text=True)
    assert r.returncode != 0 and "RuntimeError" in r.stderr and "mdm_hip.h is missing" in r.stderr, r.stderr


def test_the_parsed_tables_are_the_types_the_wrappers_rely_on():
    """Spot values written down here, not derived: scalar widths, descriptor pointers typed, every other pointer void*."""
    from mdm import _lib
    C = ctypes
    assert _lib._PROTOS["mdm_add"] == ([C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p], C.c_int32)
    assert _lib._PROTOS["mdm_gemm_pair"] == ([C.POINTER(_lib.GemmDesc)] * 2 + [C.c_void_p], C.c_int32)
    assert _lib._PROTOS["mdm_groupnorm_bwd"] == ([C.POINTER(_lib.GnDesc), C.c_void_p], C.c_int32)
    assert _lib._PROTOS["mdm_groupnorm_bwd_ws_floats"] == ([C.c_int32] * 3, C.c_int64)
    assert _lib._PROTOS["mdm_dropout_mask"][0][1] is C.c_uint64 and _lib._PROTOS["mdm_fill_f32"][0][1] is C.c_float
    assert _lib._PROTOS["mdm_last_error"] == ([], C.c_char_p) == _lib._PROTOS["mdm_gemm_last_route"] == _lib._PROTOS["mdm_attn_last_route"]
    assert _lib._PROTOS["mdm_attn_route_of"] == ([C.c_int32] * 4, C.c_char_p)
    assert _lib._PROTOS["mdm_gn_route_of"] == ([C.c_int32, C.POINTER(_lib.GnDesc)], C.c_char_p)
    assert _lib._PROTOS["mdm_gn_last_route"] == ([], C.c_char_p) and _lib._PROTOS["mdm_gn_route_names"] == ([C.c_void_p, C.c_int32], C.c_int32)
    assert dict(_lib.GnDesc._fields_)["drop_base"] is C.c_uint64 and dict(_lib.GemmDesc._fields_)["wtap"] is C.c_int64
    assert _lib._PARAMS["mdm_add"] == ["dtype", "dst", "src", "n", "stream"]
    assert _lib._PROTOS["mdm_skinny_route_of"] == ([C.c_int32] * 5, C.c_char_p) and _lib._PROTOS["mdm_skinny_last_route"] == ([], C.c_char_p)
    assert _lib._PROTOS["mdm_skinny_route_names"] == ([C.c_void_p, C.c_int32], C.c_int32)
    assert _lib._PROTOS["mdm_gemm_launch_of"] == ([C.POINTER(_lib.GemmDesc), C.c_void_p], C.c_int32)      # `int32_t out[6]`: a pointer
    assert _lib._PROTOS["mdm_gemm_pair_launch_of"] == ([C.POINTER(_lib.GemmDesc)] * 2 + [C.c_void_p], C.c_int32)
    assert len(_lib._PROTOS) == 92 and len(_lib.EXPORTS) == 92


def test_call_binds_keywords_against_the_header_names():
    """Under a Recording (nothing launches): keyword, mixed and positional calls record the same tuple; a misspelt, missing or
    doubled parameter is a TypeError naming the entry point and records nothing."""
    from mdm import _lib
    lib = _lib.load()
    with _lib.Recording() as rec:
        _lib.call("mdm_add", 0, 16, 32, 8, None)
        _lib.call("mdm_add", dtype=0, dst=16, src=32, n=8, stream=None)
        _lib.call("mdm_add", 0, 16, n=8, stream=None, src=32)
        assert rec.calls == [("mdm_add", lib.mdm_add, (0, 16, 32, 8))] * 3
        for bad in (dict(dtype=0, dest=16, src=32, n=8, stream=None),          # misspelt
                    dict(dtype=0, dst=16, src=32, stream=None)):               # missing
            with pytest.raises(TypeError, match="mdm_add"):
                _lib.call("mdm_add", **bad)
        with pytest.raises(TypeError, match="mdm_add"):                        # doubled
            _lib.call("mdm_add", 0, 16, 32, dst=16, n=8, stream=None)
        with pytest.raises(TypeError, match="mdm_add"):                        # one too many
            _lib.call("mdm_add", 0, 16, 32, 8, None, stream=None)
        assert len(rec.calls) == 3 and len(rec.keep) == 3


def _gn_desc(**kw):
    """A descriptor both GroupNorm entry points would accept (fake non-null pointers: never dereferenced on the host), then `kw`."""
    from mdm import _lib
    f = dict(dtype=_lib.BF16, N=2, P=16, G=32, C0=64, C1=0, silu=1, eps=1e-6, src0=16, gamma=16, beta=16, stats=16, y=16,
             dy=16, dst0=16, dgamma=16, dbeta=16)
    f.update(kw)
    return _lib._desc(f, _lib.GnDesc)


FWD, BWD = "mdm_groupnorm_fwd", "mdm_groupnorm_bwd"
DROP = dict(rng=16, ctl=16, drop_base=8)
GN_REFUSALS = [      # descriptor fields, entry points, substring of mdm_last_error
    (dict(dtype=7), (FWD, BWD), "bad dtype"),
    (dict(C0=60), (FWD, BWD), "channel counts must be multiples of 8"),
    (dict(C0=64, C1=8, src1=16, dst1=16), (FWD, BWD), "not divisible by G"),
    (dict(N=0), (FWD, BWD), "bad N/P"),
    (dict(C0=32, C1=32, src1=16, dst1=16, sum_all=16), (BWD,), "column sums need a single-source dx"),
    (dict(dtype=0, N=1, C0=32, P=2304), (BWD,), "the fp32 path needs ws"),
    (dict(DROP, C0=32, C1=32, src1=16, dst1=16), (FWD, BWD), "a dropout site has one source"),
    (dict(DROP, ctl=None), (FWD, BWD), "null rng / ctl"),
    (dict(DROP, drop_base=2 ** 33 + 4), (FWD, BWD), "base must be a multiple of 8"),
]


@pytest.mark.parametrize("fields,entries,message", GN_REFUSALS, ids=[m for _, _, m in GN_REFUSALS])
def test_groupnorm_refuses_bad_descriptors_on_the_host(fields, entries, message):
    """Every argument check of the two GroupNorm entry points runs before their first launch: the descriptors below come back
    non-zero with their message on a box without a device (and nothing is launched on one that has a device)."""
    from mdm import _lib
    lib = _lib.load()
    for name in entries:
        d = _gn_desc(**fields)
        assert getattr(lib, name)(ctypes.byref(d), None) != 0, name
        assert message in lib.mdm_last_error().decode(), (name, lib.mdm_last_error().decode())


def test_groupnorm_refuses_a_null_descriptor():
    from mdm import _lib
    lib = _lib.load()
    for name in (FWD, BWD):
        assert getattr(lib, name)(None, None) != 0
        assert "null descriptor" in lib.mdm_last_error().decode()


def test_groupnorm_wrappers_fill_the_descriptor():
    """What ops.groupnorm_* record (nothing launches inside a Recording): the accumulate / addend arguments become add0 / add0b /
    add1 as the C ABI defines them, drop_base keeps its 64 bits, eps defaults to 1e-6."""
    from mdm import _lib, ops
    src0, src1, gamma, beta, dy, stats, dst0, dst1, pend, pend1, dgamma, dbeta, rng, ctl, y = ts = [torch.empty(8) for _ in range(15)]
    assert len({t.data_ptr() for t in ts}) == len(ts)
    p = lambda t: None if t is None else t.data_ptr()

    def bwd(acc0, add0, acc1=0, add1=None, two=True, drop=False):
        with _lib.Recording() as rec:
            if drop:
                ops.groupnorm_bwd_dropout(_lib.BF16, src0, 64, 2, 16, gamma, beta, 1, dy, stats, dst0, acc0, dgamma, dbeta, None,
                                          rng, 2 ** 33 + 8, ctl, add0=add0, sum_ld=7)
            else:
                ops.groupnorm_bwd(_lib.BF16, src0, 32, src1 if two else None, 32 if two else 0, 2, 16, gamma, beta, 1, dy, stats,
                                  dst0, acc0, dst1 if two else None, acc1, dgamma, dbeta, None, add0=add0, add1=add1)
        (name, _, args), = rec.calls
        assert name == BWD
        d = args[0]._obj
        assert any(k[0] is d for k in rec.keep if isinstance(k, tuple))       # the recording owns the descriptor
        return d

    for drop in (False, True):
        d = bwd(1, None, drop=drop)                 # accumulate, no addend
        assert (d.dst0, d.add0, d.add0b) == (p(dst0), p(dst0), None)
        d = bwd(1, pend, drop=drop)                 # accumulate and a pending addend
        assert (d.dst0, d.add0, d.add0b) == (p(dst0), p(dst0), p(pend))
        d = bwd(0, pend, drop=drop)                 # overwrite, pending addend
        assert (d.dst0, d.add0, d.add0b) == (p(dst0), p(pend), None)
        d = bwd(0, None, drop=drop)                 # overwrite
        assert (d.dst0, d.add0, d.add0b) == (p(dst0), None, None)
    assert (d.rng, d.drop_base, d.ctl, d.sum_ld, d.C1, d.dst1, d.add1) == (p(rng), 2 ** 33 + 8, p(ctl), 7, 0, None, None)
    assert (bwd(0, None).rng, bwd(0, None).drop_base, bwd(0, None).ctl) == (None, 0, None)
    d = bwd(0, None, acc1=1)
    assert (d.dst1, d.add1) == (p(dst1), p(dst1))
    d = bwd(0, None, add1=pend1)
    assert (d.dst1, d.add1) == (p(dst1), p(pend1))
    with pytest.raises(AssertionError, match="one addend"):
        bwd(0, None, acc1=1, add1=pend1)
    d = bwd(0, None, two=False)                     # one source: a null dst1 is legal
    assert (d.C1, d.src1, d.dst1, d.add1) == (0, None, None, None)
    assert (d.src0, d.gamma, d.beta, d.dy, d.stats, d.dgamma, d.dbeta, d.ws) == \
           tuple(map(p, (src0, gamma, beta, dy, stats, dgamma, dbeta, None)))
    assert (d.dtype, d.N, d.P, d.G, d.C0, d.silu) == (_lib.BF16, 2, 16, 32, 32, 1)
    with _lib.Recording() as rec:
        ops.groupnorm_fwd(_lib.F32, src0, 32, src1, 32, 2, 16, gamma, beta, 0, y, stats, None)
        ops.groupnorm_fwd_dropout(_lib.F32, src0, 64, 2, 16, gamma, beta, 1, y, stats, None, rng, 2 ** 33 + 8, ctl)
    (n0, _, a0), (n1, _, a1) = rec.calls
    d0, d1 = a0[0]._obj, a1[0]._obj
    assert n0 == n1 == FWD and d0.eps == d1.eps == ctypes.c_float(1e-6).value
    assert (d0.y, d0.src1, d0.C1, d0.rng, d0.silu) == (p(y), p(src1), 32, None, 0)
    assert (d1.y, d1.src1, d1.C1, d1.rng, d1.drop_base, d1.ctl, d1.silu) == (p(y), None, 0, p(rng), 2 ** 33 + 8, p(ctl), 1)


def test_errors_come_back_as_exceptions_not_crashes():
    from mdm import _lib
    with pytest.raises(RuntimeError, match="bad dtype"):
        _lib.gemm(dtype=7, layout=0, M=8, N=8, K=8)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _lib.gemm(dtype=1, layout=0, M=8, N=12, K=8, D0=1, ldd0=8, A=1, B=1, lda=8, ldb=8)
    with pytest.raises(RuntimeError, match="C <= 8"):
        _lib.call("mdm_degrade", 1, None, None, None, 1, None, 1, 4, 9, 16, 1, 0, 0.0, None, None, None, None)


def test_product_fails_loudly_without_gpu():
    import mdm
    if torch.cuda.is_available():
        pytest.skip("needs a CPU-only box")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mdm.UNet(TINY, N=1, H=16, W=16)


# ------------------------------------------------------------------------------- host logic
@pytest.mark.parametrize("kind", ["linear", "log", "exponential"])
def test_scheduler_tables_match_reference(golden, kind):
    import mdm
    g = golden("schedules")
    for size in (32, 64):
        for T in (10, 50, 250, 1000):
            s = mdm.Scheduler(base_args(data_size=size, ddpm_schedule=kind, ddpm_num_steps=T), device="cpu")
            assert s.update_ddpm_num_steps(T) == int(g[f"sched_{kind}_{T}_{size}_steps"])
            assert np.array_equal(s.get_ratio_list().numpy(), g[f"sched_{kind}_{T}_{size}_ratio"])
            assert np.array_equal(np.asarray(s.get_black_area_num_pixels_all()), g[f"sched_{kind}_{T}_{size}_pixels"])


def test_scheduler_timesteps_gather_weights(golden):
    import mdm
    g = golden("schedules")
    for scale in (1, 3):
        s = mdm.Scheduler(base_args(data_size=32, ddpm_num_steps=50, scheduler_num_scale_timesteps=scale), device="cpu")
        s.update_ddpm_num_steps(50)
        for epoch in (0, 3, 5, 8):
            assert s.get_timesteps_epoch(epoch, 9) == list(g[f"epochsteps_s{scale}_e{epoch}"])
    a = base_args(data_size=32, ddpm_schedule="log", ddpm_num_steps=50, select_degrade_pixel="indexing")
    s = mdm.Scheduler(a, device="cpu")
    n = s.update_ddpm_num_steps(50)
    t = torch.from_numpy(g["gather_log_idx_t"])
    assert np.array_equal(s.get_black_area_num_pixels_time(t).numpy(), g["gather_log_idx"])
    a.select_degrade_pixel = "thresholding"
    assert np.array_equal(s.get_black_area_num_pixels_time(t.float()).numpy(), g["gather_log_thr"])
    assert np.array_equal(s.get_weight_timesteps(torch.tensor([0, 1, 7, n - 1]), 10.0).numpy(), g["lossw"])
    with pytest.raises(TypeError):
        mdm.Scheduler(base_args(ddpm_schedule="sigmoid"), device="cpu").update_ddpm_num_steps(10)
    with pytest.raises(ValueError):
        mdm.Scheduler(base_args(ddpm_schedule="cosine"), device="cpu").update_ddpm_num_steps(10)


def test_each_scheduler_kernel_is_launched_from_one_place():
    """One statement of every quirk: `Scheduler.emit_shift` / `emit_degrade` hold the only calls of their kernels, `per_column`,
    the `SHIFT_KINDS` lookup and `_fill_mode` live in scheduler.py alone (DESIGN finding 60)."""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "masked-diffusion-model_amd", "mdm")
    text = {f: open(os.path.join(pkg, f)).read() for f in sorted(os.listdir(pkg)) if f.endswith(".py")}
    where = lambda needle: {f: t.count(needle) for f, t in text.items() if needle in t}
    for needle in ('"mdm_shift"', '"mdm_degrade"', '"mdm_index_mask"', "per_column=", "SHIFT_KINDS["):
        assert where(needle) == {"scheduler.py": 1}, (needle, where(needle))
    assert set(where("_fill_mode(")) == {"scheduler.py"}
    assert "_shift_draws" not in "".join(text.values()) and "def _kind" not in text["train_step.py"]


@pytest.mark.parametrize("rows", [None, (1, 3, 4)])
def test_scheduler_host_draws_consume_the_generator_like_the_reference(rows):
    """The three replay-mode helpers draw for the WHOLE batch in the reference's order and shape and keep this rank's rows:
    'noise_with_perturbation' consumes one uniform draw that it discards (D11), 'noise_std_reduction' draws image by image."""
    import mdm
    n = 4
    lo, hi = (0, n) if rows is None else rows[:2]
    ratio = torch.linspace(0.1, 0.9, n, dtype=torch.float64)

    def sched(**kw):
        s = mdm.Scheduler(base_args(data_size=4, noise_mean=0.25, **kw), device="cpu")
        s.replay_rows = rows
        return s
    s = sched(shift_type="noise_with_perturbation")
    torch.manual_seed(7)
    z = s.host_shift_z(ratio, hi - lo, 3, 4, 4)
    torch.manual_seed(7)
    torch.empty(n, 1, 1, 1).uniform_(-1.0, 1.0)
    want = torch.empty(n, 3, 4, 4).normal_(mean=0.25, std=1)
    assert torch.equal(z, want[lo:hi]) and z.is_contiguous()
    after = torch.get_rng_state()
    torch.manual_seed(7)
    s.host_shift_z(ratio, hi - lo, 3, 4, 4)
    assert torch.equal(torch.get_rng_state(), after)

    s = sched(shift_type="noise_std_reduction")
    torch.manual_seed(8)
    z = s.host_shift_z(ratio, hi - lo, 3, 4, 4)
    torch.manual_seed(8)
    want = torch.stack([torch.empty(1, 3, 4, 4).normal_(mean=0.25, std=float(r))[0] for r in ratio])
    assert torch.equal(z, want[lo:hi])
    assert sched(shift_type="non_shift").host_shift_z(ratio, hi - lo, 3, 4, 4) is None

    s = sched(degrade_channel="3-channel")
    torch.manual_seed(9)
    u = s.host_uniforms(torch.zeros(hi - lo, 3, 4, 4))
    torch.manual_seed(9)
    assert torch.equal(u, torch.empty(n, 3 * 16).uniform_(0.0, 1.0)[lo:hi])

    counts = torch.tensor([0, 5, 16, 9])
    torch.manual_seed(10)
    m = s.host_index_mask(counts, hi - lo, 3, 4, 4)
    torch.manual_seed(10)
    perms = [torch.randperm(16) for _ in range(n)]
    assert m.shape == (hi - lo, 3, 4, 4) and torch.equal((m[:, 0] == 0).flatten(1).sum(1), counts[lo:hi])
    for k, i in enumerate(range(lo, hi)):
        assert set(torch.nonzero(m[k, 1].flatten() == 0).flatten().tolist()) == set(perms[i][:counts[i]].tolist())
    assert torch.equal(s._host_full(counts[lo:hi], hi - lo), counts[lo:hi] if rows is None else counts[lo:lo + 1].expand(n))


def test_state_dict_grammar_and_layout_roundtrip():
    from mdm.unet import ParamStore, UNet, unet6_config
    from oracle.unet_ref import param_shapes, random_params, unet6_config as ref_cfg
    for cfg, hw in ((TINY, 16), (unet6_config(32), 32)):
        table = UNet.param_table(cfg, hw, hw)
        ref = param_shapes(cfg)
        assert set(table) == set(ref) and all(tuple(table[k]) == tuple(ref[k]) for k in ref)
    assert unet6_config(64) == ref_cfg(64) and unet6_config(256) == ref_cfg(256)
    assert sum(int(np.prod(v)) for v in UNet.param_table(unet6_config(32)).values()) == 35746307
    net = UNet(TINY, 1, 16, 16, _dry=True)
    st = net.store
    p = random_params(TINY, 3)
    for k in p:                                  # OIHW <-> [tap][O_p][I_p] and the channel padding
        back = st.to_reference(k, st.to_internal(k, p[k]))
        assert torch.equal(back, p[k]), k
    w = st.to_internal("in_conv.weight", p["in_conv.weight"])
    assert w.shape == (9, 32, 8) and float(w[:, :, 3:].abs().sum()) == 0
    assert torch.equal(w[4, :, :3], p["in_conv.weight"][:, :, 1, 1])
    # all time-embedding projections sit back to back (one contraction for the 22 of them)
    offs = [st.entries[k + ".weight"].off for k in net.fc_slots]
    sizes = [st.entries[k + ".weight"].n for k in net.fc_slots]
    assert all(offs[i] + sizes[i] == offs[i + 1] for i in range(len(offs) - 1))


def test_bucket_planning():
    from mdm.dist import GradComm
    marks = [(10, 900), (20, 600), (30, 590), (45, 100), (50, 0)]
    cuts, buckets = GradComm.plan_buckets(marks, 1000, 300)
    assert buckets[0][1] == 1000 and buckets[-1][0] == 0
    assert all(buckets[i][0] == buckets[i + 1][1] for i in range(len(buckets) - 1))        # tile [0, total)
    assert cuts == sorted(cuts) and len(cuts) == len(buckets) and cuts[-1] == 50
    assert all(hi - lo >= 300 for lo, hi in buckets[:-1])
    cuts1, b1 = GradComm.plan_buckets(marks, 1000, 10 ** 9)                                   # one bucket
    assert b1 == [(0, 1000)] and cuts1 == [50]
    net_marks = [(5, 7), (9, 0)]
    assert GradComm.plan_buckets(net_marks, 8, 1) == ([5, 9], [(7, 8), (0, 7)])
    # tapered tail: the exposed last exchange shrinks geometrically, the plan still tiles [0, total)
    fine = [(k, 1000 - 10 * k) for k in range(1, 101)]
    c2, b2 = GradComm.plan_buckets(fine, 1000, 300, tail_elems=40)
    assert b2[0][1] == 1000 and b2[-1][0] == 0 and all(b2[i][0] == b2[i + 1][1] for i in range(len(b2) - 1))
    sizes = [hi - lo for lo, hi in b2]
    assert sizes[0] >= 300 and sizes[-1] <= 80 and len(b2) > len(GradComm.plan_buckets(fine, 1000, 300)[1])


def test_ema_and_lr_schedules_per_call_site_arguments():
    from mdm.optim import EMA, get_lr_scheduler
    from oracle.trainer_ref import ema_decay

    class _M:        # EMA only touches .store.P here
        class store:
            P = torch.zeros(4)
    e = EMA(_M, decay=0.9999, inv_gamma=1.0, power=0.75)
    assert e.get_decay(1) == 0.0
    for k in (2, 10, 1000, 10 ** 7):
        assert abs(e.get_decay(k) - ema_decay(k)) < 1e-12
    assert e.get_decay(10 ** 9) == 0.9999

    class _O:
        param_groups = [dict(lr=1.0, initial_lr=1.0)]
    for name in ("constant", "linear", "cosine", "hard_cosine"):
        o = _O()
        o.param_groups = [dict(lr=1.0, initial_lr=1.0)]
        s = get_lr_scheduler(name, o, 10, 100)
        lrs = []
        for _ in range(100):
            lrs.append(s.get_last_lr()[0])
            s.step()
        assert lrs[0] == 0.0 and abs(lrs[5] - 0.5) < 1e-9 and abs(lrs[10] - 1.0) < 1e-9
        assert all(0.0 <= v <= 1.0 for v in lrs)
        if name in ("linear", "cosine"):
            assert lrs[-1] < 0.1


# ------------------------------------------------------------------------------- data parallel over gloo
_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "masked-diffusion-model_amd")); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch, torch.distributed as dist
from mdm.dist import GradComm, init_from_env
from golden.make_golden import TINY
from oracle.unet_ref import UNetRef, random_params
init_from_env("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
torch.manual_seed(0)
# (a) bucketed exchange of a flat buffer == one big all-reduce
comm = GradComm(bucket_bytes=4 * 300)
marks = [(3, 700), (5, 400), (9, 0)]
cuts, comm.buckets = GradComm.plan_buckets(marks, 1000, comm.bucket_bytes // 4)
flat = torch.arange(1000, dtype=torch.float32) * (rank + 1)
for i in range(len(comm.buckets)):
    comm.reduce_bucket(i, flat)
comm.wait_all()
want = torch.arange(1000, dtype=torch.float32) * sum(r + 1 for r in range(world))
assert torch.equal(flat, want), "bucketed all-reduce"
# (a') the same through the bf16 wire format (values chosen exactly representable: the sums must be exact too)
comm3 = GradComm(bucket_bytes=4 * 300, wire="bf16")
comm3.buckets = [(500, 1000), (0, 500)]
flat = (torch.arange(1000) % 64).float() * (rank + 1)
for i in range(2):
    comm3.reduce_bucket(i, flat)
comm3.wait_all(flat)
assert torch.equal(flat, (torch.arange(1000) % 64).float() * sum(r + 1 for r in range(world))), "bf16-wire all-reduce"
# (b) DP gradient equivalence on the oracle model: mean over ranks of shard-mean grads == full-batch grad
g = torch.Generator().manual_seed(5)
x = torch.rand(4, 3, 16, 16, generator=g) * 2 - 1
t = torch.tensor([3.0, 9.0, 1.0, 7.0])
tgt = torch.rand(4, 3, 16, 16, generator=g)
def flat_grad(xs, ts, ys):
    m = UNetRef(TINY, random_params(TINY))
    loss = ((m(xs, ts).sample - ys) ** 2).mean()
    loss.backward()
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()])
full = flat_grad(x, t, tgt)
sl = slice(rank * 2, rank * 2 + 2)
mine = flat_grad(x[sl], t[sl], tgt[sl])
comm2 = GradComm(bucket_bytes=1 << 16)
n = mine.numel()
comm2.buckets = [(n // 2, n), (0, n // 2)]
for i in range(2):
    comm2.reduce_bucket(i, mine)
comm2.wait_all()
mine *= 1.0 / world                      # the optimizer kernel's gmul
err = float((mine - full).norm() / full.norm())
assert err < 1e-5, err
dist.barrier()
if rank == 0:
    print("DP_OK", err)
dist.destroy_process_group()
'''


def test_data_parallel_exchange_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert "DP_OK" in outs[0]


# ------------------------------------------------------------------------------------------- bench.py contract
def _run_bench(args, env_extra, timeout=300):
    env = dict(os.environ, **env_extra)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if k not in env_extra:
            env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_bench_refuses_a_job_size_other_than_gpus():
    r = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], dict(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0 and "--gpus 2 but WORLD_SIZE=3" in r.stderr and not r.stdout.strip()


def test_bench_has_full_and_dump_outputs_and_refuses_zero_steps():
    r = _run_bench(["--help"], {})
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stdout[-2000:]
    r = _run_bench(["--steps", "0"], {})
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr and not r.stdout.strip(), r.stderr[-2000:]


def test_bench_gpus_n_starts_n_ranks_itself():
    """No GPU here: both ranks must come up (through torch.distributed.run) and each fail loudly at the
    no-CPU-fallback check -- proof that `python bench.py --gpus 2` is not a one-rank no-op any more."""
    if torch.cuda.is_available():
        pytest.skip("CPU-only check (the GPU variant lives in tests/test_dp_gpu.py)")
    r = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-sampler"], {})
    assert r.returncode != 0 and not r.stdout.strip()
    assert r.stderr.count("bench.py needs a GPU") >= 2, r.stderr[-2000:]


def test_sampler_shard_bounds_and_gather_gloo_world2(tmp_path):
    from mdm.sampler import shard_bounds
    for n, w in ((100, 8), (5, 2), (7, 7), (3, 4)):
        b = [shard_bounds(n, r, w) for r in range(w)]
        assert b[0][0] == 0 and b[-1][1] == n and all(b[i][1] == b[i + 1][0] for i in range(w - 1))
        sizes = [hi - lo for lo, hi in b]
        assert max(sizes) - min(sizes) <= 1 and sorted(sizes, reverse=True) == sizes
    worker = tmp_path / "w.py"
    worker.write_text(r'''
import os, sys
ROOT = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, "masked-diffusion-model_amd"))
import torch, torch.distributed as dist
from mdm.dist import init_from_env
from mdm.sampler import gather_shards, shard_bounds
init_from_env("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
n = 5
lo, hi = shard_bounds(n, rank, world)
full = torch.arange(n * 6, dtype=torch.float32).reshape(n, 2, 3)
got = gather_shards(full[lo:hi].clone(), n)
assert torch.equal(got, full), (rank, got)
if rank == 0:
    print("GATHER_OK")
dist.barrier(); dist.destroy_process_group()
''')
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(worker), ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=120)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert "GATHER_OK" in outs[0]


def test_reference_param_order_is_the_modules_registration_order():
    from mdm.unet import UNet, unet6_config
    from oracle.unet_ref import param_shapes
    for cfg in (unet6_config(32), dict(in_channels=4, hid_channels=32, out_channels=4, ch_multipliers=[1, 2, 2],
                                       num_res_blocks=1, apply_attn=[True, True, True])):
        assert UNet(cfg, 1, 32, 32, _dry=True).reference_param_order() == list(param_shapes(cfg))


def test_groupnorm_bwd_workspace_size_on_the_host():
    """mdm_groupnorm_bwd_ws_floats is host logic (no launch): fp32 needs 3 x N x C floats, bf16 none."""
    from mdm import _lib
    lib = _lib.load()
    assert lib.mdm_groupnorm_bwd_ws_floats(_lib.F32, 4, 256) == 3 * 4 * 256 and lib.mdm_groupnorm_bwd_ws_floats(_lib.BF16, 4, 256) == 0
