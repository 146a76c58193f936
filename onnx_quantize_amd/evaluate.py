"""How good is the quantized file?  Sliding-window perplexity of an ONNX causal LM on the device.

The device counterpart of the reference's ``tools/perplexity.py`` (which runs an onnxruntime session over wikitext): the model
runs through `GraphRunner`, by default with its MatMulNBits nodes on the fused kernel (`ops.matmul_nbits`: from the blob as stored,
no expanded weight), and the windows, the shift and the count of targets are the reference's.  Tokenising stays the caller's
business -- this package ships no tokenizer: hand in the token ids.
"""
from __future__ import annotations

import math
import os

import numpy as np

from .onnx_proto import Message, load_model, parse_model

__all__ = ["perplexity", "perplexity_windows"]


def perplexity_windows(length: int, max_length: int, stride: int):
    """The windows of tools/perplexity.py as (begin, end, counted): `begin` runs over range(0, length, stride), `end` is
    min(begin + max_length, length), `counted` = end - previous end is the number of newly revealed targets the window scores
    (never more than its end - begin - 1 predictions); the walk stops at end == length."""
    if max_length < 2 or stride < 1:
        raise ValueError(f"perplexity: max_length >= 2 and stride >= 1 are needed, got {max_length} and {stride}")
    prev_end = 0
    for begin in range(0, length, stride):
        end = min(begin + max_length, length)
        yield begin, end, min(end - prev_end, end - begin - 1)
        prev_end = end
        if end == length:
            break


def _as_model(model) -> Message:
    if isinstance(model, Message):
        return model
    if isinstance(model, (bytes, bytearray, memoryview)):
        return parse_model(bytes(model))
    if isinstance(model, (str, os.PathLike)):
        return load_model(model)
    raise TypeError(f"perplexity: model must be a path, bytes or a parsed ModelProto, got {type(model).__name__}")


def perplexity(model, input_ids, *, max_length: int = 2048, stride: int = 512, extra_feeds=None, device="cuda",
               matmul_nbits: str = "fused", qlinear: str = "torch", qdq: str = "torch") -> float:
    """exp(mean negative log-likelihood) of ``input_ids`` (1-D integers) under the causal LM ``model`` (a path, bytes or a parsed
    ModelProto), over the sliding windows of `perplexity_windows`.

    Each window feeds ``input_ids`` [1, n] int64 and, when the model declares them, ``attention_mask`` (ones) and
    ``position_ids`` (0 ... n - 1).  ``extra_feeds`` -- a dict, or a callable of the window length n returning one -- supplies
    every other declared input (empty past-key tensors, say); a declared input nobody feeds raises by name.  The logits are the
    output named ``logits``, or the model's single output; position t predicts token t + 1.  Log-softmax and the sum of the
    negative log-likelihoods run in float64 on the device, and one scalar comes back to the host per call, not per window.

    ``matmul_nbits`` goes to `GraphRunner` as it is: "fused+decode" sends the MatMulNBits nodes of windows of at most 16 tokens to the
    decode kernel (`ops.matmul_nbits_decode`: HQQ files and block size 16 included); "fused+float_zp" and "fused+float_zp+decode"
    also run the nodes of an HQQ file (floating-point zero points, block sizes that are multiples of 32) from the blob at any
    window length (`ops.matmul_nbits_float_zp`), where "fused" expands their weight per call.  The default stays "fused".

    ``qlinear="fused"`` runs the QLinearMatMul / QGemm nodes of a `format="qlinear"` file on the int8 matrix cores
    (`ops.qlinear_matmul`: exact int32 sums).  The default stays the expansion route: a fused output may differ from it by one
    output level, where the expansion's fp32 sum lands on the other side of a rounding boundary.  ``qlinear="fused+decode"`` goes to
    `GraphRunner` as it is: the nodes of windows of at most 16 tokens run on the decode kernel (`ops.qlinear_matmul_decode`), with
    the bytes of ``"fused"``.  ``qlinear="function"`` and ``"function+decode"`` go to `GraphRunner` as they are too: every call of the
    file's QLinearMatMul / QLinearGemm functions -- QuantizeLinear, the integer product, DequantizeLinear -- runs as one library call
    (`ops.qlinear_function`; windows of at most 16 tokens on `ops.qlinear_function_decode` under ``"function+decode"``), with the bytes
    of ``"fused"``, so the perplexity is the same number.

    ``qdq="fused"`` runs the product of every `quant`-domain QDQ function call -- the default output format -- from the stored
    integers (`ops.qdq_matmul`: no fp32 copy of the weight is made per call).  The default stays the function body: the fused sum
    differs from torch's fp32 GEMM on the dequantized weight in its last bits.  ``qdq="fused+integer"`` also runs every call of a QDQ
    function with an input Q -> DQ (static or dynamic activations) as one library call on the int8 matrix cores (`ops.qdq_function`:
    an exact int32 sum where the other routes accumulate the dequantized activations in fp32)."""
    import torch

    from .graph_runner import GraphRunner

    ids = np.asarray(input_ids)
    if ids.ndim != 1 or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"perplexity: input_ids must be a 1-D integer array, got shape {ids.shape} of {ids.dtype}")
    if len(ids) < 2:
        raise ValueError("perplexity: at least two tokens are needed (one prediction)")
    proto = _as_model(model)
    outputs = [o.name for o in proto.graph.output]
    if "logits" in outputs:
        wanted = "logits"
    elif len(outputs) == 1:
        wanted = outputs[0]
    else:
        raise ValueError(f"perplexity: the model has outputs {outputs}, none of them named 'logits'")
    runner = GraphRunner(proto, outputs=[wanted], device=device, matmul_nbits=matmul_nbits, qlinear=qlinear, qdq=qdq)
    if "input_ids" not in runner.input_names:
        raise ValueError(f"perplexity: the model declares no input 'input_ids' (inputs: {runner.input_names})")
    dev = runner.device
    tokens = torch.from_numpy(ids.astype(np.int64)).to(dev)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    counted_all = 0
    for begin, end, counted in perplexity_windows(len(ids), max_length, stride):
        n = end - begin
        if counted <= 0:
            continue
        feeds = {"input_ids": tokens[begin:end].reshape(1, n)}
        if "attention_mask" in runner.input_names:
            feeds["attention_mask"] = torch.ones((1, n), dtype=torch.int64, device=dev)
        if "position_ids" in runner.input_names:
            feeds["position_ids"] = torch.arange(n, dtype=torch.int64, device=dev).reshape(1, n)
        extra = extra_feeds(n) if callable(extra_feeds) else extra_feeds
        for name, value in (extra or {}).items():
            if name not in runner.input_names:
                raise ValueError(f"perplexity: extra feed '{name}' is not an input of the model (inputs: {runner.input_names})")
            feeds[name] = value
        unfed = [name for name in runner.input_names if name not in feeds]
        if unfed:
            raise ValueError(f"perplexity: model input '{unfed[0]}' is fed by nobody -- pass it through extra_feeds")
        logits = runner(feeds)[wanted]
        logits = logits.reshape(-1, logits.shape[-1])
        if logits.shape[0] != n:
            raise ValueError(f"perplexity: {n} tokens went in, logits for {logits.shape[0]} positions came out")
        scored = torch.log_softmax(logits[n - 1 - counted:n - 1].to(torch.float64), dim=-1)
        targets = tokens[end - counted:end]
        total -= scored.gather(1, targets.reshape(-1, 1)).sum()
        counted_all += counted
    return math.exp(float(total) / counted_all)
