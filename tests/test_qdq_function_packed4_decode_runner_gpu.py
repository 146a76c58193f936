"""`GraphRunner(qdq="fused+integer+packed4+decode")`: the calls "fused+integer+packed4" sends to `ops.qdq_function_packed4` go to
`ops.qdq_function_packed4_decode` where the flattened X has at most 16 rows.  The file is the two-layer one of
test_qdq_function_packed4_runner_gpu.py: a static-input MatMul feeding a dynamic-input Gemm, and an odd-N call that walks the body."""
import pytest
import torch

from onnx_quantize_amd.graph_runner import GraphRunner
from test_qdq_function_packed4_runner_gpu import K, two_layers

pytestmark = pytest.mark.gpu
MODE = "fused+integer+packed4+decode"


def feed_of(rows):
    return {"x": torch.randint(-2, 3, (rows, K), generator=torch.Generator().manual_seed(rows)).float()}


@pytest.mark.parametrize("rows,counts", [(5, {"integer": 0, "body": 1, "packed4": 0, "decode": 2}), (17, {"integer": 0, "body": 1, "packed4": 2, "decode": 0})])
def test_up_to_16_rows_take_the_decode_kernel_and_give_the_tile_routes_bytes(rows, counts):
    model, feed = two_layers(), feed_of(rows)
    decode, tile = GraphRunner(model, device="cuda", qdq=MODE), GraphRunner(model, device="cuda", qdq="fused+integer+packed4")
    assert decode.qdq == MODE and decode.qdq_function_calls == dict.fromkeys(counts, 0) and "decode" not in tile.qdq_function_calls
    a, b = decode(feed), tile(feed)
    assert decode.qdq_function_calls == counts and tile.qdq_function_calls == {"integer": 0, "body": 1, "packed4": 2}
    for name in ("out", "odd"):
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name
        assert float(b[name].abs().max()) > 1.0


def test_a_decode_pass_is_recordable_and_a_cpu_runner_stays_on_torch():
    model, feed = two_layers(), feed_of(5)
    eager, rec = GraphRunner(model, device="cuda", qdq=MODE), GraphRunner(model, outputs=["out"], device="cuda", qdq=MODE, capture=True)
    want = eager(feed)["out"].view(torch.int32)
    for i in range(4):
        assert torch.equal(rec(feed)["out"].view(torch.int32), want), i
    assert next(iter(rec._graphs.values())) is not None, "a pass on the decode route synchronises with nothing: it can be recorded"
    assert rec.qdq_function_calls["decode"] >= 2 and rec.qdq_function_calls["body"] == 0
    assert GraphRunner(model, device="cpu", qdq=MODE).qdq == "torch"
