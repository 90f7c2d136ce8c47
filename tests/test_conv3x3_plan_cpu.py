"""conv_plan.conv3x3_plan against tests/golden/conv3x3_paths.json: the `ops` wrappers one Conv3x3Fn forward + backward
went through on an MI355X, recorded with conv_path_checks.run_conv on the commit BEFORE the plan existed (the inline
ladders of dpt_engine), for the 20 table rows and for every 3x3 layer of the models at bench.py's batch sizes.  A
threshold that moves shows up here as a fixture row that moves."""
import glob
import os

import pytest
import torch

import conv_path_checks as chk
from ssl4gie_amd import _lib, conv_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = chk.load_fixture()


def expected_calls(plan, relu_in):
    """the fixed table: plan entry -> wrappers, in call order"""
    fwd = {"direct": [chk.flagged("conv3x3_direct_fwd", plan.fwd_stats, False)],
           "gather": [chk.flagged("conv3x3_fwd", plan.fwd_stats, False)],
           "im2col": ["im2col3x3", "linear_fwd"]}[plan.fwd]
    # one fresh fp32 target and a fresh bias target: the bias gradient rides on the product (no colsum), and the
    # weight gradient is scattered by conv3x3_wgrad_unpack
    wgrad = {"direct": ["conv3x3_direct_wgrad"],
             "gather": ["conv3x3_bwd_weight"],
             "im2col": ["im2col3x3", "linear_bwd_weight"]}[plan.wgrad] + ["conv3x3_wgrad_unpack"]
    # direct and gather mask the gradient by the ReLU in front in their epilogue; the other two need relu_bwd
    dgrad = {"direct": [chk.flagged("conv3x3_direct_fwd", False, relu_in)],
             "gather": [chk.flagged("conv3x3_fwd", False, relu_in)],
             "im2col": ["im2col3x3", "linear_fwd"] + ["relu_bwd"] * relu_in,
             "col2im": ["linear_bwd_data", "col2im3x3"] + ["relu_bwd"] * relu_in}[plan.dgrad]
    return fwd, wgrad + dgrad


def test_fixture_holds_the_table_and_the_model_layers():
    assert [tuple(r["row"]) for r in FIXTURE[:20]] == chk.ROWS
    sources = {r["source"] for r in FIXTURE[20:]}
    assert {"depth", "moco", "det", "convstem_small", "convstem_base", "faster_rcnn"} <= sources


@pytest.mark.parametrize("i", range(len(FIXTURE)))
def test_plan_gives_the_recorded_calls(i):
    rec = FIXTURE[i]
    B, H, W, Ci, Co, stride, dtype, bias, want_stats, relu_in = rec["row"]
    plan = conv_plan.conv3x3_plan(B, H, W, Ci, Co, stride, chk.DTYPES[dtype], bias, want_stats)
    fwd, bwd = expected_calls(plan, relu_in)
    assert (fwd, bwd) == (rec["fwd"], rec["bwd"]), (rec["source"], plan)
    assert plan.ld == conv_plan.k_pad(9 * Ci, chk.DTYPES[dtype]) and plan.ld2 == conv_plan.k_pad(9 * Co, chk.DTYPES[dtype])
    if plan.fwd_stats:
        assert want_stats and not bias


def test_table_rows_take_the_paths_worked_out_by_hand():
    """the cross-check of the recording: (fwd, statistics from the kernel, wgrad, dgrad) of rows 1-20"""
    hand = [("direct", True, "direct", "direct"), ("gather", True, "gather", "im2col"),
            ("gather", True, "im2col", "col2im"), ("im2col", True, "im2col", "col2im"),
            ("im2col", True, "gather", "col2im"), ("direct", False, "direct", "direct"),
            ("gather", False, "gather", "gather"), ("im2col", False, "gather", "im2col"),
            ("direct", False, "im2col", "direct"), ("direct", False, "gather", "direct"),
            ("im2col", False, "gather", "im2col"), ("gather", False, "gather", "gather"),
            ("im2col", False, "im2col", "col2im"), ("direct", False, "direct", "gather"),
            ("gather", False, "gather", "im2col"), ("im2col", False, "gather", "gather"),
            ("im2col", False, "im2col", "im2col"), ("direct", False, "direct", "direct"),
            ("im2col", False, "im2col", "im2col"), ("im2col", False, "im2col", "col2im")]
    for row, want in zip(chk.ROWS, hand):
        B, H, W, Ci, Co, stride, dtype, bias, want_stats, _ = row
        p = conv_plan.conv3x3_plan(B, H, W, Ci, Co, stride, chk.DTYPES[dtype], bias, want_stats)
        assert (p.fwd, p.fwd_stats, p.wgrad, p.dgrad) == want, row


def test_limit_functions_agree_with_the_library():
    lib = _lib.load()
    chans = (8, 24, 32, 64, 96, 128, 256, 512, 544)
    for Ci in chans:
        for Co in chans:
            for W in (1, 2, 16, 17):
                g = (3, 5, W, Ci, Co)
                assert conv_plan.direct_fwd_ok(*g, torch.bfloat16) == bool(lib.ssl4gie_conv3x3_direct_ok(*g)), g
                assert conv_plan.direct_wgrad_ok(*g, torch.bfloat16) == \
                    bool(lib.ssl4gie_conv3x3_direct_wgrad_ok(*g)), g
                assert not conv_plan.direct_fwd_ok(*g, torch.float32)
                assert not conv_plan.direct_wgrad_ok(*g, torch.float32)
                # what the C side states in words (conv_direct.hip): 32-channel passes, 8 couts per store; the
                # weight gradient in 64-channel slices and 32-cout groups up to 512
                assert conv_plan.direct_fwd_ok(*g, torch.bfloat16) == (Ci % 32 == 0 and Co % 8 == 0), g
                assert conv_plan.direct_wgrad_ok(*g, torch.bfloat16) == \
                    (Ci % 64 == 0 and Co % 32 == 0 and Ci <= 512 and Co <= 512), g


def test_operand_cache_state_lives_in_lpcache_only():
    """the derived-operand cache is LPCache's: nothing outside engine.py reaches into it"""
    banned = ("lp._c", "._c[", "._c.", "_conv_recipes", "_conv_epoch", "lp.__dict__", "lp_cache.__dict__",
              "cache.__dict__")
    files = glob.glob(os.path.join(ROOT, "ssl4gie_amd", "**", "*.py"), recursive=True) + \
        glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True) + [os.path.join(ROOT, "bench.py")]
    assert len(files) > 20
    for path in files:
        if os.path.relpath(path, ROOT) == os.path.join("ssl4gie_amd", "engine.py"):
            continue
        with open(path) as f:
            src = f.read()
        for word in banned:
            assert word not in src, (os.path.relpath(path, ROOT), word)
