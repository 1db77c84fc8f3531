"""Every export of include/mdm_hip.h has a test at kernel level, or launches no kernel of its own.

COVERAGE maps each symbol of `_lib._PROTOS` to (test module, what that module calls it by): the symbol itself where the test goes
through the C ABI, or the `ops` / `_lib` wrapper it calls.  "host only": the entry point computes on the host (a predicate, a route
query, a plan, error text) or wraps the HIP runtime (graphs, events, streams) -- its tests are wherever its callers are.  A new export
without a row fails here; so does a row whose module no longer mentions the call."""
import os
import re

from mdm import _lib

HOST = "host only"
_G, _A, _H, _T, _D = "test_gemm_routes_gpu", "test_attn_routes_gpu", "test_helper_kernels_gpu", "test_temb_bounds_gpu", "test_device_draws_gpu"
_S, _L, _E = "test_store_kernels_gpu", "test_loss_sampler_kernels_gpu", "test_eval_kernels_gpu"

COVERAGE = {
    "mdm_last_error": HOST, "mdm_version": HOST, "mdm_device_count": HOST,
    "mdm_gemm": (_G, "_lib.gemm"), "mdm_gemm_pair": ("test_kernels_gpu", "mdm_gemm_pair"),
    "mdm_gemm_plan": HOST, "mdm_gemm_can_fuse_gn_bwd": HOST, "mdm_gemm_can_fuse_gn_fwd": HOST, "mdm_gemm_last_route": HOST,
    "mdm_gemm_route_of": HOST, "mdm_gemm_pair_route_of": HOST, "mdm_gemm_launch_of": HOST, "mdm_gemm_pair_launch_of": HOST,
    "mdm_gemm_route_names": HOST,
    "mdm_wgrad_group_accepts": HOST, "mdm_wgrad_group_create": HOST, "mdm_wgrad_group_schedule": HOST,
    "mdm_wgrad_group_launch": ("test_wgrad_group_gpu", "_lib.WgradGroup"), "mdm_wgrad_group_destroy": HOST,
    "mdm_conv_wgrad_split": ("test_grad_split_gpu", "mdm_conv_wgrad_split"), "mdm_conv_wgrad_split_plan": HOST,
    "mdm_wgrad_split_last_route": HOST,
    "mdm_groupnorm_fwd": ("test_gn_bounds_gpu", "mdm_groupnorm_fwd"), "mdm_groupnorm_bwd": ("test_gn_bounds_gpu", "mdm_groupnorm_bwd"),
    "mdm_gn_route_of": HOST, "mdm_gn_last_route": HOST, "mdm_gn_route_names": HOST, "mdm_groupnorm_bwd_ws_floats": HOST,
    "mdm_dropout_mask": ("test_dropout_gpu", "ops.dropout_mask"),
    "mdm_attn_supported": HOST, "mdm_attn_route_of": HOST, "mdm_attn_last_route": HOST, "mdm_attn_route_names": HOST,
    "mdm_attn_f32_small_supported": HOST,
    "mdm_attn_f32_small_fwd": (_A, "ops.attn_f32_small_fwd"), "mdm_attn_fwd": (_A, "ops.attn_fwd"), "mdm_attn_bwd": (_A, "ops.attn_bwd"),
    "mdm_attn_mh_fwd": (_A, "ops.attn_mh_fwd"), "mdm_attn_mh_bwd": (_A, "ops.attn_mh_bwd"),
    "mdm_softmax_fwd": (_A, "ops.softmax_fwd"), "mdm_softmax_bwd": (_A, "ops.softmax_bwd"),
    "mdm_timestep_embedding": (_H, "ops.timestep_embedding"), "mdm_timestep_embedding2": (_H, "ops.timestep_embedding"),
    "mdm_silu_fwd": (_H, "ops.silu_fwd"), "mdm_silu_bwd": (_H, "ops.silu_bwd"),
    "mdm_skinny_route_of": HOST, "mdm_skinny_last_route": HOST, "mdm_skinny_route_names": HOST, "mdm_skinny_supported": HOST,
    "mdm_skinny_linear_fwd": (_T, "mdm_skinny_linear_fwd"), "mdm_skinny_linear_bwd": (_T, "mdm_skinny_linear_bwd"),
    "mdm_silu_bwd_sum": (_T, "mdm_silu_bwd_sum"),
    "mdm_colsum": (_H, "ops.colsum"), "mdm_sumpool2": (_H, "ops.sumpool2"), "mdm_avgpool2": (_H, "ops.avgpool2"),
    "mdm_upsample2": (_H, "ops.upsample2"), "mdm_add": (_H, "ops.add_"), "mdm_add3": (_H, "ops.add3"),
    "mdm_nchw_to_nhwc": (_H, "ops.nchw_to_nhwc"), "mdm_nhwc_to_nchw": (_H, "ops.nhwc_to_nchw"),
    "mdm_draw_timesteps": (_D, "mdm_draw_timesteps"), "mdm_degrade": (_D, "mdm_degrade"), "mdm_index_mask": (_D, "mdm_index_mask"),
    "mdm_shift": (_D, "mdm_shift"), "mdm_zero_pad_channels": ("test_kernels_gpu", "mdm_zero_pad_channels"),
    "mdm_loss_fwd_bwd": (_L, "mdm_loss_fwd_bwd"), "mdm_loss_fwd_bwd_mon": ("test_monitor_gpu", "mdm_loss_fwd_bwd_mon"),
    "mdm_monitor_commit": ("test_monitor_gpu", "mdm_monitor_commit"),
    "mdm_sampler_x0": (_L, "mdm_sampler_x0"), "mdm_rng_advance": (_D, "mdm_rng_advance"),
    "mdm_sampler_step_params": (_D, "mdm_sampler_step_params"), "mdm_sampler_update": (_L, "mdm_sampler_update"),
    "mdm_normalize01": (_E, "mdm_normalize01"), "mdm_unit_rows": (_E, "mdm_unit_rows"), "mdm_col_argmax": (_E, "mdm_col_argmax"),
    "mdm_sqnorm": (_S, "mdm_sqnorm"), "mdm_optim_update": ("test_optimizers_gpu", "mdm_optim_update"),
    "mdm_cast_bf16": (_S, "mdm_cast_bf16"), "mdm_transpose_shadow_bf16": (_S, "mdm_transpose_shadow_bf16"),
    "mdm_split_shadow": (_S, "mdm_split_shadow"), "mdm_split_shadow_t": (_S, "mdm_split_shadow_t"),
    "mdm_fill_f32": (_S, "mdm_fill_f32"), "mdm_fill_segments_f32": (_S, "mdm_fill_segments_f32"),
    "mdm_graph_begin": HOST, "mdm_graph_end": HOST, "mdm_graph_launch": HOST, "mdm_graph_destroy": HOST,
    "mdm_event_create": HOST, "mdm_event_record": HOST, "mdm_event_elapsed_ms": HOST, "mdm_event_destroy": HOST, "mdm_stream_sync": HOST,
}
TESTS = os.path.dirname(os.path.abspath(__file__))


def test_the_table_names_every_export_and_nothing_else():
    missing, extra = sorted(set(_lib._PROTOS) - set(COVERAGE)), sorted(set(COVERAGE) - set(_lib._PROTOS))
    assert not missing, f"exports of include/mdm_hip.h without a row (add a kernel-level test and name it here): {missing}"
    assert not extra, f"rows for symbols the header no longer declares: {extra}"


def test_every_named_module_mentions_its_call():
    texts = {}
    for sym, where in COVERAGE.items():
        if where == HOST:
            continue
        mod, mention = where
        path = os.path.join(TESTS, mod + ".py")
        assert os.path.exists(path), (sym, mod)
        if mod not in texts:
            with open(path) as fh:
                texts[mod] = fh.read()
        assert re.search(r"(?<![\w.])" + re.escape(mention) + r"\b", texts[mod]), f"{mod}.py does not mention {mention} ({sym})"
        assert "pytest.mark.gpu" in texts[mod], f"{mod}.py is named for {sym} but holds no GPU tests"


def test_a_wrapper_the_table_names_calls_the_symbol_it_stands_for():
    """`ops.f` / `_lib.f` rows: the wrapper's source names the symbol"""
    import inspect

    from mdm import ops
    for sym, where in COVERAGE.items():
        if where == HOST or where[1].startswith("mdm_"):
            continue
        owner, fn = where[1].split(".")
        src = inspect.getsource(getattr({"ops": ops, "_lib": _lib}[owner], fn))
        assert sym in src, (sym, where)
