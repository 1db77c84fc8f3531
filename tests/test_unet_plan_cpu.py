"""The U-Net's launch plan (`UNet._plan`) on `_dry` nets: no GPU, the host predicates of the cross-compiled library only.

Structural invariants of the decisions, their counts per net and mode against literals (see EXPECT for where they come from),
and two guards on the source of mdm/unet.py and mdm/unet2d.py that keep emission (`fwd` / `bwd`) from deciding anything again."""
import ast
import os

import pytest

import mdm
from mdm.unet import _AttnCore, _Conv, _Norm
from mdm.unet2d import UNet2D, my_model_config

BF16, F32 = mdm.BF16, mdm.F32
TINY = dict(in_channels=3, hid_channels=32, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[False, True])
CFG4 = dict(in_channels=4, hid_channels=128, out_channels=4, ch_multipliers=[1, 2, 2, 2], num_res_blocks=2, apply_attn=[True] * 4)
NETS = {"tiny_n4_16": (mdm.UNet, TINY, 4, 16), "cfg2_n32": (mdm.UNet, mdm.unet6_config(32), 32, 32),
        "cfg3_n8": (mdm.UNet, mdm.unet6_config(64), 8, 64), "cfg4_n16": (mdm.UNet, CFG4, 16, 32),
        "unet2d_n4": (UNet2D, my_model_config(3, 32, num_attention=1), 4, 32)}
MODES = {"bf16": BF16, "f32": F32}
CASES = [(n, m) for n in NETS for m in MODES]

# Decision counts per net and mode.  They are MEANT to be the counts of the PARENT commit 52be3d3 ("gemm: choose the route in a pure host
# function, launch from one switch"), read off the launches it recorded on an MI355X: `scripts/plan_fingerprint.py --summary` of its
# fingerprint file (fp_parent.json of profiles/r07_plan_emit_split.md) -- call names and descriptor fields, nothing this code computes.
# UNVERIFIED AGAINST HARDWARE: no MI355X could be had while this was written.  The figures below were read off the PARENT's own recorded
# plans all the same, in a host rehearsal: the parent's constructors recording onto host tensors (every launch outside a recording
# skipped, the group handle faked), fingerprinted by the script and summarised with --summary.  They are not figures of the planning
# pass; the same rehearsal of this change gave byte-identical fingerprints for all 36 nets it covered (profiles/r07_plan_emit_split.md).
# To verify on hardware: run the script on a checkout of 52be3d3, compare its --summary with this table, then drop this paragraph.
# Columns: GroupNorm forwards run as a conv epilogue (descriptors with gnf_out), GroupNorm backwards run as a data-gradient epilogue
# (gnb_x), mdm_gemm_pair launches of the forward / of the backward, weight gradients inside a group launch / on mdm_conv_wgrad_split /
# as a launch of their own, convs whose sums a norm emits (sum_all of mdm_groupnorm_bwd_add, gnb_sum_all), mdm_attn_fwd launches.
COLUMNS = ("gn_fwd_fused", "gn_bwd_fused", "fwd_pairs", "bwd_pairs", "wgrad_grouped", "wgrad_split", "wgrad_single", "sums_by_norm",
           "attn_fused")
EXPECT = {
    ("tiny_n4_16", "bf16"): (0, 0, 5, 5, 33, 0, 0, 8, 4),
    ("tiny_n4_16", "f32"): (0, 0, 0, 0, 0, 0, 33, 8, 0),
    ("cfg2_n32", "bf16"): (22, 24, 13, 13, 77, 0, 0, 22, 6),
    ("cfg2_n32", "f32"): (0, 0, 0, 0, 0, 0, 77, 22, 0),
    ("cfg3_n8", "bf16"): (11, 12, 13, 13, 76, 0, 1, 22, 6),
    ("cfg3_n8", "f32"): (0, 0, 0, 0, 0, 0, 77, 22, 0),
    ("cfg4_n16", "bf16"): (27, 29, 13, 13, 107, 0, 0, 22, 21),
    ("cfg4_n16", "f32"): (0, 0, 0, 0, 0, 0, 107, 22, 0),
    ("unet2d_n4", "bf16"): (12, 14, 0, 0, 62, 0, 58, 32, 0),
    ("unet2d_n4", "f32"): (0, 0, 0, 0, 0, 0, 120, 32, 0),
}

_cache = {}


def planned(name, dt, **kw):
    key = (name, dt, tuple(sorted(kw.items())))
    if key not in _cache:
        cls, cfg, n, hw = NETS[name]
        net = cls(cfg, n, hw, hw, dtype=dt, _dry=True, **kw)
        net._plan()
        _cache[key] = net
    return _cache[key]


def convs(net):
    return [s for s in net.specs if isinstance(s, _Conv)]


def norms(net):
    return [s for s in net.specs if isinstance(s, _Norm)]


def counts(net):
    cs, ns = convs(net), norms(net)
    return dict(gn_fwd_fused=sum(n.fwd_fused for n in ns), gn_bwd_fused=sum(n.bwd_fused for n in ns),
                fwd_pairs=sum(c.fwd_mate is not None for c in cs), bwd_pairs=sum(c.bwd_mate is not None for c in cs),
                wgrad_grouped=sum(c.wgrad == "grouped" for c in cs), wgrad_split=sum(c.wgrad == "split" for c in cs),
                wgrad_single=sum(c.wgrad == "single" for c in cs), sums_by_norm=sum(c.sums == "norm" for c in cs),
                attn_fused=sum(s.mode == "fused" for s in net.specs if isinstance(s, _AttnCore)))


@pytest.mark.parametrize("name,mode", CASES)
def test_decision_counts_match_the_parents_launches(name, mode):
    got = counts(planned(name, MODES[mode]))
    assert got == dict(zip(COLUMNS, EXPECT[name, mode])), got


@pytest.mark.parametrize("name,mode", CASES)
def test_structure_of_the_plan(name, mode):
    dt = MODES[mode]
    net = planned(name, dt)
    specs, cs = net.specs, convs(net)
    for n in norms(net):
        k = specs.index(n)
        host = [c for c in cs if c.gn_fwd is n]
        assert len(host) == int(n.fwd_fused)
        if n.fwd_fused:                     # the conv immediately before it, single source, that conv's output
            assert host[0] is specs[k - 1] and n.src1 is None and host[0].out is n.src0
        users = [c for c in cs if c.src0 is n.out or c.src1 is n.out]
        if n.bwd_fused:                     # the producer of the ONLY source of every conv that reads it
            assert users and all(c.gn_bwd is n and c.src1 is None and c.src0.norm_spec is n for c in users)
        else:
            assert not any(c.gn_bwd is n for c in cs)
    for c in cs:
        assert c.gn_bwd is None or (c.src0.norm_spec is c.gn_bwd and c.src1 is None)
        # exactly one source of bias sums, and each kind only where it can exist
        assert c.sums in ("colsum", "wgrad", "norm")
        assert (c.sums == "norm") == (c.block is not None and c.block.conv1 is c and c.block.norm2.sums_for is c)
        assert c.sums != "wgrad" or (dt == BF16 and c.fc_slot is None)
        assert c.wgrad in ("grouped", "split", "single") and (c.dgrad is None) == (not c.src0.needs_grad)
    assert sum(n.sums_for is not None for n in norms(net)) == sum(c.sums == "norm" for c in cs)
    # a skip projection is in exactly one forward pair iff pairing is on and the net is bf16 (UNet2D stays unpaired)
    pairing = dt == BF16 and net.pair_convs and net.pair_blocks
    for b in net.blocks:
        assert b.conv1.block is b and b.norm2.block is b and b.conv2.block is b and (b.skip is None or b.skip.block is b)
        if b.skip is not None:
            assert [c for c in cs if c.fwd_mate is b.skip] == ([b.conv1] if pairing else [])
            assert b.skip.fwd_in_pair == pairing
            assert [c for c in cs if c.bwd_mate is b.skip] == ([b.conv2] if pairing else [])
            assert b.skip.bwd_in_pair == pairing
    assert sum(c.fwd_in_pair for c in cs) == sum(c.fwd_mate is not None for c in cs)
    if dt == F32:                           # nothing that only exists for bf16
        assert not any(n.fwd_fused or n.bwd_fused for n in norms(net))
        assert not any(c.fwd_mate or c.bwd_mate or c.gn_fwd or c.gn_bwd or c.fwd_in_pair or c.bwd_in_pair for c in cs)
        assert all(c.wgrad != "grouped" and c.sums != "wgrad" and c.dgrad != "t" for c in cs)
        assert all(s.mode != "fused" for s in specs if isinstance(s, _AttnCore))


def test_pairing_off_plans_no_pairs():
    net = planned("cfg2_n32", BF16, pair_convs=False)
    assert not any(c.fwd_mate or c.bwd_mate or c.fwd_in_pair or c.bwd_in_pair for c in convs(net))
    on = planned("cfg2_n32", BF16)
    assert [c.gn_fwd is None for c in convs(net)] == [c.gn_fwd is None for c in convs(on)]


def test_ungrouped_plans_no_group():
    net = planned("cfg2_n32", BF16, group_wgrads=False)
    assert all(c.wgrad == "single" for c in convs(net))


def test_split_gradients_follow_split_grad_reason():
    from mdm import ops
    net = planned("cfg2_n32", F32, f32_products="split", grad_products="split")
    for c in convs(net):
        rw, rd = ops.split_grad_reason(c.g, "wgrad"), ops.split_grad_reason(c.g, "dgrad")
        assert c.wgrad == ("split" if rw is None else "single")
        want = {} if rw is None else {"wgrad": "exact:" + rw}
        if c.src0.needs_grad:
            assert c.dgrad == ("split" if rd is None else "exact")
            if rd is not None:
                want["dgrad"] = "exact:" + rd
        assert c.grad_exact == want
    assert all(c.grad_exact == {} for c in convs(planned("cfg2_n32", F32)))


@pytest.mark.parametrize("mode", list(MODES))
def test_uniform_t_plans_have_no_backward_decisions(mode):
    net = planned("cfg2_n32", MODES[mode], uniform_t=True)
    for c in convs(net):
        assert (c.sums, c.wgrad, c.dgrad, c.gn_bwd, c.bwd_mate, c.bwd_in_pair, c.grad_exact) == (None, None, None, None, None, False, {})
    assert not any(n.bwd_fused or n.sums_for is not None for n in norms(net))
    full = planned("cfg2_n32", MODES[mode])             # ... and the forward decisions of the full plan
    assert [(c.fwd_in_pair, c.fwd_mate is not None, c.gn_fwd is not None) for c in convs(net)] == \
           [(c.fwd_in_pair, c.fwd_mate is not None, c.gn_fwd is not None) for c in convs(full)]


# ---- guards on the source: emission reads the plan, it does not write decisions -----------------------------------------------
SOURCES = [os.path.join(os.path.dirname(mdm.__file__), f) for f in ("unet.py", "unet2d.py")]
EMITTERS = {"fwd", "bwd", "_fwd_fields", "fwd_epilogue", "sums_fields", "_note_route"}
OWN_BUFFERS = {"stats", "lse", "S", "delta", "e", "h1", "a1", "tm", "st_"}       # what a spec allocates for itself while it is emitted
ACT_GRAD_STATE = {"grad", "grad_written", "pending_add"}                         # gradient-buffer bookkeeping of an activation


def _attr_targets(fn):
    for node in ast.walk(fn):
        tgts = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, (ast.AugAssign, ast.AnnAssign)) else []
        for t in tgts:
            for leaf in ast.walk(t):
                if isinstance(leaf, ast.Attribute) and isinstance(leaf.ctx, ast.Store):
                    yield leaf


@pytest.mark.parametrize("path", SOURCES)
def test_emission_assigns_no_decision_and_nothing_on_another_spec(path):
    """Emitting the forward / backward twice over the same spec objects gives the same launches: a `fwd` / `bwd` body (and the helpers
    they call on a spec) stores only the buffers that spec allocates for itself, and the gradient bookkeeping of activations."""
    tree, seen = ast.parse(open(path).read()), 0
    for cls in [n for n in tree.body if isinstance(n, ast.ClassDef)]:
        for fn in [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in EMITTERS]:
            seen += 1
            for t in _attr_targets(fn):
                own = isinstance(t.value, ast.Name) and t.value.id == "self" and t.attr in OWN_BUFFERS
                assert own or t.attr in ACT_GRAD_STATE, f"{os.path.basename(path)}:{t.lineno} {cls.name}.{fn.name} assigns .{t.attr}"
    assert seen >= 2


@pytest.mark.parametrize("path", SOURCES)
def test_no_getattr_with_a_default(path):
    """Links and optional buffers are declared fields: a typo fails instead of silently switching a fusion off."""
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "getattr":
            assert len(node.args) < 3 and not node.keywords, f"{os.path.basename(path)}:{node.lineno} getattr with a default"
