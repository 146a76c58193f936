"""What `runner_routes` decides, pinned without a GPU: the accepted strings, the counters' keys, the order of the routes of every
mode, the plan of every QDQ function, which 4-bit weights are held packed, and the identity tables.  Every expected value is written
out here; none is computed from the tables under test.  A runner over a model with no initializers can be built for "cuda" without a
GPU (nothing is uploaded), which is how the counters of the GPU-only modes are read."""
import itertools

import numpy as np
import pytest
import torch

from onnx_quantize_amd import onnx_proto as P
from onnx_quantize_amd.graph_runner import GraphRunner
from onnx_quantize_amd.onnx_functions import _QDQ, build_function
from onnx_quantize_amd.runner_routes import NBITS_MODES, QLINEAR_MODES, ById, _QdqPlan, _unpacked4, first_route

OPSETS = [P.Message("OperatorSetIdProto", domain="", version=21), P.Message("OperatorSetIdProto", domain="quant", version=1)]
EMPTY = P.Message("ModelProto", ir_version=10, graph=P.Message("GraphProto", name="g"), opset_import=OPSETS)
ACCEPTED = {"matmul_nbits": ["torch", "fused", "fused+decode", "fused+float_zp", "fused+float_zp+decode"],
            "qlinear": ["torch", "fused", "fused+decode", "function", "function+decode"],
            "qdq": ["torch", "fused", "fused+integer", "fused+packed4", "fused+integer+packed4"]}


@pytest.mark.parametrize("keyword", list(ACCEPTED))
def test_accepted_strings_read_torch_on_the_host_and_a_misspelling_is_refused(keyword):
    for mode in ACCEPTED[keyword]:
        assert getattr(GraphRunner(EMPTY, device="cpu", **{keyword: mode}), keyword) == "torch"
        assert getattr(GraphRunner(EMPTY, device="cuda", **{keyword: mode}), keyword) == mode
    for device in ("cpu", "cuda"):
        with pytest.raises(ValueError, match=keyword):
            GraphRunner(EMPTY, device=device, **{keyword: ACCEPTED[keyword][-1] + "s"})
    with pytest.raises(ValueError, match=r"fused\+packed4"):
        GraphRunner(EMPTY, device="cpu", qdq="packed4")


BASE = dict(nbits_calls={"fused": 0, "torch": 0}, qlinear_calls={"fused": 0, "torch": 0}, qlinear_function_calls={"function": 0, "body": 0},
            qdq_calls={"fused": 0, "torch": 0}, qdq_function_calls={"integer": 0, "body": 0})
EXTRA = {("matmul_nbits", "fused+decode"): dict(nbits_calls=["decode"]), ("matmul_nbits", "fused+float_zp"): dict(nbits_calls=["float_zp"]),
         ("matmul_nbits", "fused+float_zp+decode"): dict(nbits_calls=["float_zp", "decode"]),
         ("qlinear", "fused+decode"): dict(qlinear_calls=["decode"]),
         ("qlinear", "function+decode"): dict(qlinear_calls=["decode"], qlinear_function_calls=["decode"]),
         ("qdq", "fused+packed4"): dict(qdq_calls=["packed4"]),
         ("qdq", "fused+integer+packed4"): dict(qdq_calls=["packed4"], qdq_function_calls=["packed4"])}


@pytest.mark.parametrize("keyword,mode", [(k, m) for k in ACCEPTED for m in ACCEPTED[k]])
def test_counter_keys_per_mode(keyword, mode):
    runner, host = GraphRunner(EMPTY, device="cuda", **{keyword: mode}), GraphRunner(EMPTY, device="cpu", **{keyword: mode})
    for name, base in BASE.items():
        expected = dict(base, **{key: 0 for key in EXTRA.get((keyword, mode), {}).get(name, [])})
        assert getattr(runner, name) == expected and type(getattr(runner, name)) is dict, name
        assert getattr(host, name) == base, name


# mode -> the routes in the order they are asked; whatever no route takes goes to "torch" (nodes) / "body" (QLinear function calls)
NBITS_ORDER = {"torch": [], "fused": ["fused"], "fused+decode": ["decode", "fused"], "fused+float_zp": ["fused", "float_zp"],
               "fused+float_zp+decode": ["decode", "fused", "float_zp"]}
QLINEAR_NODE_ORDER = {"torch": [], "fused": ["fused"], "fused+decode": ["decode", "fused"], "function": ["fused"], "function+decode": ["decode", "fused"]}
QLINEAR_CALL_ORDER = {"torch": [], "fused": [], "fused+decode": [], "function": ["function"], "function+decode": ["decode", "function"]}


def subsets(names):
    return [set(c) for r in range(len(names) + 1) for c in itertools.combinations(names, r)]


def test_the_first_route_that_accepts_wins_in_every_mode():
    assert set(NBITS_MODES) == set(NBITS_ORDER) and set(QLINEAR_MODES) == set(QLINEAR_NODE_ORDER)
    for mode, order in NBITS_ORDER.items():
        for accepting in subsets(["decode", "fused", "float_zp"]):
            expected = next((r for r in order if r in accepting), "torch")
            assert first_route(NBITS_MODES[mode], lambda r: r in accepting, "torch") == expected, (mode, accepting)
    for mode in QLINEAR_MODES:
        for accepting in subsets(["decode", "fused", "function"]):
            node = next((r for r in QLINEAR_NODE_ORDER[mode] if r in accepting), "torch")
            call = next((r for r in QLINEAR_CALL_ORDER[mode] if r in accepting), "body")
            assert first_route(QLINEAR_MODES[mode][0], lambda r: r in accepting, "torch") == node, (mode, accepting)
            assert first_route(QLINEAR_MODES[mode][1], lambda r: r in accepting, "body") == call, (mode, accepting)
    # spelled out
    assert first_route(NBITS_MODES["fused+float_zp+decode"], lambda r: r == "float_zp", "torch") == "float_zp"
    assert first_route(NBITS_MODES["fused+float_zp+decode"], lambda r: r in ("decode", "fused"), "torch") == "decode"
    assert first_route(NBITS_MODES["fused+float_zp"], lambda r: r == "decode", "torch") == "torch"
    assert first_route(NBITS_MODES["fused"], lambda r: r == "float_zp", "torch") == "torch"
    assert first_route(QLINEAR_MODES["function"][0], lambda r: True, "torch") == "fused"
    assert first_route(QLINEAR_MODES["function+decode"][1], lambda r: r == "function", "body") == "function"
    assert first_route(QLINEAR_MODES["fused+decode"][1], lambda r: True, "body") == "body"


# name -> ((sorted weight_nodes, product, x, bias, group_size), input_mode)
MATMUL_IN, MATMUL_PLAIN = ([0], 3, "x_dequantized", None, 0), ([0], 1, "X", None, 0)
GEMM_IN, GEMM_PLAIN = ([0], 4, "x_dequantized", "dequantized_bias", 0), ([0], 2, "X", "dequantized_bias", 0)
PLANS = {"QGemmWeightDynamicInputOutputQDQ": (GEMM_IN, "dynamic"), "QGemmWeightDynamicInputQDQ": (GEMM_IN, "dynamic"),
         "QGemmWeightDynamicOutputQDQ": (GEMM_PLAIN, None), "QGemmWeightInputOutputQDQ": (GEMM_IN, "static"),
         "QGemmWeightInputQDQ": (GEMM_IN, "static"), "QGemmWeightOutputQDQ": (GEMM_PLAIN, None), "QGemmWeightsOnlyQDQ": (GEMM_PLAIN, None),
         "QMatMulWeightDynamicInputOutputQDQ": (MATMUL_IN, "dynamic"), "QMatMulWeightDynamicInputQDQ": (MATMUL_IN, "dynamic"),
         "QMatMulWeightDynamicOutputQDQ": (MATMUL_PLAIN, None), "QMatMulWeightStaticInputOutputQDQ": (MATMUL_IN, "static"),
         "QMatMulWeightStaticInputQDQ": (MATMUL_IN, "static"), "QMatMulWeightStaticOutputQDQ": (MATMUL_PLAIN, None),
         "QMatMulWeightsOnlyQDQ": (MATMUL_PLAIN, None)}
GROUPED = {("QMatMulWeightsOnlyGrouped", False): ([0, 1, 2, 3, 4, 5], 6, "X", None, 32),
           ("QMatMulWeightsOnlyGrouped", True): ([0, 1, 2, 3, 4, 5, 6, 7], 8, "X", None, 32),
           ("QGemmWeightsOnlyGrouped", False): ([0, 1, 2, 3, 4, 5], 7, "X", "dequantized_bias", 32),
           ("QGemmWeightsOnlyGrouped", True): ([0, 1, 2, 3, 4, 5, 6, 7], 9, "X", "dequantized_bias", 32)}


def plan_of(fn):
    p = _QdqPlan.of(fn)
    return None if p is None else (sorted(p.weight_nodes), p.product, p.x, p.bias, p.group_size)


def test_the_plan_of_every_qdq_function():
    assert set(PLANS) == set(_QDQ)
    for name, (plan, mode) in PLANS.items():
        fn = build_function(name)
        assert plan_of(fn) == plan and _QdqPlan.input_mode(fn) == mode and _QdqPlan.named(fn), name
    for (name, four_bit), plan in GROUPED.items():
        fn = build_function(name, group_size=32, four_bit=four_bit)
        assert plan_of(fn) == plan and _QdqPlan.input_mode(fn) is None and _QdqPlan.named(fn), (name, four_bit)


def test_a_body_that_is_not_the_writers_has_no_plan():
    def altered(change, name="QGemmWeightInputOutputQDQ", **kw):
        fn = P.parse_model(P.serialize(P.Message("ModelProto", ir_version=10, graph=P.Message("GraphProto", name="g"), functions=[build_function(name, **kw)],
                                                 opset_import=OPSETS))).functions[0]
        assert plan_of(fn) is not None                         # through the wire it is still the writer's
        change(fn)
        return plan_of(fn)

    def one_attribute(fn):
        gemm = next(n for n in fn.node if n.op_type == "Gemm")
        gemm.attribute = list(gemm.attribute) + [P.make_node("x", [], [], alpha=0.5).attribute[0]]

    def swapped(fn):
        fn.node[0].input = list(fn.node[0].input)[::-1]

    def extra_node(fn):
        fn.node = list(fn.node) + [P.make_node("Identity", ["out"], ["out2"])]

    def other_domain(fn):
        fn.domain = "quant2"

    def no_block(fn):
        dq = next(n for n in fn.node if n.op_type == "DequantizeLinear" and any(a.name == "block_size" for a in n.attribute))
        dq.attribute = [a for a in dq.attribute if a.name != "block_size"] + [P.make_node("x", [], [], block_size=0).attribute[0]]

    def two_blocked(fn):
        dq = next(n for n in fn.node if n.op_type == "DequantizeLinear" and any(a.name == "block_size" for a in n.attribute))
        fn.node = list(fn.node) + [dq.copy()]

    for change in (one_attribute, swapped, extra_node, other_domain):
        assert altered(change) is None, change.__name__
    for change in (no_block, two_blocked):
        assert altered(change, "QMatMulWeightsOnlyGrouped", group_size=32) is None, change.__name__


K, N1, N2, N3 = 64, 48, 34, 33
FUNCTIONS = ["QMatMulWeightStaticInputQDQ", "QGemmWeightDynamicInputQDQ"]


def two_layers(extra_nodes=(), outputs=("out", "odd"), first_inputs=None, dims=None, functions=None, unread=False):
    """The model of test_qdq_function_packed4_runner_gpu.py (W1 INT4 [64, 48], W2 UINT4 [48, 34], W3 INT4 [48, 33]), with one thing
    changed per variant."""
    rng = np.random.default_rng(5)
    inits = []

    def weight(name, k, n, code):
        lo, box = (-8, np.int8) if code == P.DataType.INT4 else (0, np.uint8)
        shape = dims.get(name, (k, n)) if dims else (k, n)
        inits.extend([P.numpy_to_tensor(name, rng.integers(lo, lo + 16, shape).astype(box), code), P.numpy_to_tensor(name + "_s", np.ones(n, np.float32)),
                      P.numpy_to_tensor(name + "_z", rng.integers(lo, lo + 16, n).astype(box), code)])
        return [name, name + "_s", name + "_z"]

    w1, w2, w3 = weight("W1", K, N1, P.DataType.INT4), weight("W2", N1, N2, P.DataType.UINT4), weight("W3", N1, N3, P.DataType.INT4)
    if unread:
        weight("W4", K, N1, P.DataType.INT4)
    inits.extend([P.numpy_to_tensor("B", rng.integers(-8, 9, N2).astype(np.int8)), P.numpy_to_tensor("B_s", np.float32(1.0)), P.numpy_to_tensor("B_z", np.int8(0)),
                  P.numpy_to_tensor("x_s", np.float32(1.0)), P.numpy_to_tensor("x_z", np.uint8(128)),
                  P.numpy_to_tensor("h_s", np.float32(0.5)), P.numpy_to_tensor("h_z", np.uint8(128))])
    nodes = [P.make_node(FUNCTIONS[0], first_inputs or ["x", *w1, "x_s", "x_z"], ["h"], domain="quant"),
             P.make_node(FUNCTIONS[1], ["h", w2[0], "B", *w2[1:], "B_s", "B_z"], ["out"], domain="quant"),
             P.make_node(FUNCTIONS[0], ["h", *w3, "h_s", "h_z"], ["odd"], domain="quant"), *extra_nodes]
    g = P.Message("GraphProto", name="two_layers", node=nodes, initializer=inits, input=[P.make_value_info("x", P.DataType.FLOAT, ["M", K])],
                  output=[P.make_value_info(o, P.DataType.FLOAT, None) for o in outputs])
    model = P.Message("ModelProto", ir_version=10, graph=g, functions=functions or [build_function(f) for f in FUNCTIONS], opset_import=OPSETS)
    return P.parse_model(P.serialize(model))


def test_which_four_bit_weights_are_held_packed():
    def packable(model, **kw):
        return GraphRunner(model, device="cpu", **kw)._packable_weights()

    assert packable(two_layers()) == {"W1", "W2"}                                                          # W3 has an odd N
    assert packable(two_layers(extra_nodes=[P.make_node("Cast", ["W1"], ["c"], to=1)])) == {"W2"}            # also read by a plain node
    assert packable(two_layers(outputs=("out", "odd", "W1"))) == {"W2"}                                     # a graph output
    assert packable(two_layers(), outputs=["out", "W2"]) == {"W1"}                                          # among `outputs=`
    assert packable(two_layers(first_inputs=["x", "W1", "W1_s", "W1", "x_s", "x_z"])) == {"W2"}             # passed twice to one call
    assert packable(two_layers(first_inputs=["x", "W3", "W1_s", "W1_z", "x_s", "W1"])) == {"W2"}            # passed in a slot that is not W
    runner = GraphRunner(two_layers(), device="cpu")                   # (no runner is built over bytes that are in another file)
    next(t for t in runner.graph.initializer if t.name == "W1").data_location = 1
    assert runner._packable_weights() == {"W2"}                                                             # external data
    assert packable(two_layers(dims={"W1": (0, N1)})) == {"W2"}                                             # an axis of no elements
    assert packable(two_layers(dims={"W1": (2, K // 2, N1)})) == {"W2"}                                     # three axes
    changed = build_function(FUNCTIONS[0])
    changed.node = list(changed.node) + [P.make_node("Identity", ["out"], ["out2"])]
    assert packable(two_layers(functions=[changed, build_function(FUNCTIONS[1])])) == {"W2"}                # the body is not the writer's
    assert packable(two_layers(unread=True)) == {"W1", "W2"}                                               # W4: nothing reads it


def test_nibbles_unpack_low_first_into_the_types_container():
    w = torch.tensor([[0x70, 0x8F, 0x12, 0x00], [0xFF, 0x08, 0x80, 0x77], [0x0F, 0xF0, 0x78, 0x87]], dtype=torch.uint8)
    signed, unsigned = _unpacked4(w, (8, True)), _unpacked4(w, (8, False))
    assert signed.dtype == torch.int8 and unsigned.dtype == torch.uint8
    assert signed.tolist() == [[0, 7, -1, -8, 2, 1, 0, 0], [-1, -1, -8, 0, 0, -8, 7, 7], [-1, 0, 0, -1, -8, 7, 7, -8]]
    assert unsigned.tolist() == [[0, 7, 15, 8, 2, 1, 0, 0], [15, 15, 8, 0, 0, 8, 7, 7], [15, 0, 0, 15, 8, 7, 7, 8]]


def test_an_identity_table_never_answers_for_another_object():
    table, made = ById(), []

    def make(obj):
        made.append(obj)
        return [len(made)]

    a, other, stranger = torch.zeros(2), torch.zeros(2), torch.zeros(2)
    first = table.memo(a, make)
    assert table.memo(a, make) is first and table.value(a) is first and made == [a]            # a hit: the same value object
    table[id(other)] = (stranger, "stale")                                                     # `other` at an id another object had
    assert table.value(other) is None and table.value(other, "no") == "no"
    assert table.memo(other, make) == [2] and made[1] is other and table.value(other) == [2]   # a miss: made anew, the entry replaced
    assert table.value(stranger) is None


def test_held_is_identity_on_the_runners_device():
    model = two_layers()
    mine = torch.full((N2,), 2, dtype=torch.int8)
    runner = GraphRunner(model, device="cpu", constants={"B": mine})
    assert runner.constants["B"] is mine and runner._held(mine)
    assert runner._held(runner.constants["W1"]) and not runner._held(runner.constants["W1"].clone())
    assert not runner._held(mine.clone()) and not runner._held(None) and not runner._held(3)
    assert torch.equal(mine.clone(), mine)


def test_an_evaluator_is_a_whole_runner():
    evaluator = GraphRunner.evaluator(21)
    assert set(vars(evaluator)) == set(vars(GraphRunner(two_layers(), device="cpu")))
    assert evaluator.opset == 21 and evaluator.device.type == "cpu" and evaluator.qdq == evaluator.qlinear == evaluator.matmul_nbits == evaluator.matmul == "torch"
    a, b = np.arange(6, dtype=np.float32).reshape(2, 3), np.arange(12, dtype=np.float32).reshape(3, 4)
    out, = evaluator.evaluate(P.make_node("MatMul", ["a", "b"], ["y"]), [a, b])
    assert np.array_equal(out, a @ b)
