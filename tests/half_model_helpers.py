"""Helpers shared by tests/test_rtn_half_abi.py and tests/test_rtn_half_gpu.py: one-chain MatMul models of one element type and
the oracle on the fp32 upcast of a weight as numeric provider."""
import numpy as np


def half_model(w_list, elem=None):
    """X [N, K0] -> MatMul(W0) -> MatMul(W1) ...: constant weights of one element type."""
    from onnx_quantize_amd.onnx_proto import DataType, Message, make_node, make_value_info, numpy_to_tensor

    elem = elem if elem is not None else (DataType.FLOAT16 if w_list[0].dtype == np.float16 else DataType.FLOAT)
    nodes, inits, cur = [], [], "X"
    for i, w in enumerate(w_list):
        out = "Y" if i == len(w_list) - 1 else f"H{i}"
        nodes.append(make_node("MatMul", [cur, f"W{i}"], [out], name=f"fc{i}"))
        inits.append(numpy_to_tensor(f"W{i}", w))
        cur = out
    g = Message("GraphProto", name="half", node=nodes, initializer=inits,
                input=[make_value_info("X", elem, ["N", int(w_list[0].shape[0])])],
                output=[make_value_info("Y", elem, ["N", int(w_list[-1].shape[1])])])
    return Message("ModelProto", ir_version=10, graph=g, opset_import=[Message("OperatorSetIdProto", domain="", version=21)])


def upcasting_oracle(value, cfg, out, nbits):
    """The oracle on the fp32 upcast of the weight: the definition of the result on a half-precision matrix."""
    from onnx_model_helpers import oracle_weight_arrays
    from onnx_quantize_amd.emission import _Value
    return oracle_weight_arrays(_Value(value.name, value.const_value.numpy().astype(np.float32)), cfg, out, nbits)
