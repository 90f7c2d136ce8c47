"""dpt_engine.Conv3x3Fn on the 20 geometries of conv_path_checks.ROWS (between them every branch of
conv_plan.conv3x3_plan): the `ops` wrappers a forward + backward goes through are exactly those recorded in
tests/golden/conv3x3_paths.json before the plan existed, and in the same run the output and the three gradients equal
the fp64 shifted-product reference.  Operands are integers in {0, 1} x {-1, 0, 1} (bias in [-2, 2]): at most
9 * 768 terms per output and 50 176 pixels per weight gradient, every sum stays below 2^24, so bf16 results are the
RNE rounding of the exact value, fp32 results the exact value itself, and the comparison is torch.equal."""
import pytest
import torch

import conv_path_checks as chk

pytestmark = pytest.mark.gpu
FIXTURE = chk.load_fixture()[:len(chk.ROWS)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


@pytest.mark.parametrize("i", range(len(chk.ROWS)))
def test_conv3x3_row_takes_the_recorded_path_and_is_exact(i):
    row, rec = chk.ROWS[i], FIXTURE[i]
    assert tuple(rec["row"]) == row
    B, H, W, Ci, Co, stride, dtype, bias, want_stats, relu_in = row
    dt = chk.DTYPES[dtype]
    fwd, bwd, t = chk.run_conv(row)
    assert fwd == rec["fwd"], f"row {i + 1} forward"
    assert bwd == rec["bwd"], f"row {i + 1} backward"

    x, w, dy = t["x"], t["w"], t["dy"]
    ref = chk.conv_ref(x, w.double(), stride)  # x >= 0: the ReLU in front is the identity on the values ...
    if bias:
        ref = ref + t["b"].double()
    assert t["y"].dtype == dt and torch.equal(t["y"], ref.to(dt)), f"forward: max diff {(t['y'].double() - ref).abs().max()}"
    if want_stats and not bias and dt == chk.BF:   # the producer's partials (their values: test_gpu_resnet.py)
        assert t["stats"].dtype == torch.float32 and t["stats"].shape[1:] == (2, Co)
    else:
        assert t["stats"] is None
    refw = chk.conv_wgrad_ref(dy, x, stride)
    assert torch.equal(t["dw"].double(), refw), f"weight gradient: max diff {(t['dw'].double() - refw).abs().max()}"
    if bias:
        assert torch.equal(t["db"].double(), dy.double().sum((0, 1, 2))), "bias gradient"
    # data gradient = full correlation of dy with the flipped kernel (stride 1) / its strided scatter (stride 2);
    # ... and its mask passes everything where x > 0, nothing where x == 0
    wf = w.double().flip(2, 3).transpose(0, 1).contiguous()
    if stride == 1:
        refx = chk.conv_ref(dy, wf, 1)
    else:
        up = torch.zeros(B, H, W, Co, dtype=chk.BF, device=chk.DEV)
        up[:, ::2, ::2] = dy
        refx = chk.conv_ref(up, wf, 1)
    if relu_in:
        refx = refx * (x > 0)
    assert torch.equal(t["dx"], refx.to(dt)), f"data gradient: max diff {(t['dx'].double() - refx).abs().max()}"
