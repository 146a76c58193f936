"""Which nodes and function calls of a quantized file `GraphRunner` hands to a library kernel (`hip.ops`) instead of expanding them
with torch: the mode tables, the predicates and the calls.  Routes run on the GPU only: on another device every mode reads "torch",
nothing is packed and the counters keep their base keys.  A replayed graph counts its recording only.  A node's mode is an ordered
tuple of routes: the first whose predicate takes the node runs it, else the operator's torch expansion does ("torch").  Every route
wants its operands on the GPU and the weight side held: constants of the model, by identity.

matmul = "pieces": products of fp32 activations with a LARGE constant weight go through the library's fp16-piece GEMM
    (`ops.matmul_pieces`: the Hessian kernels' arithmetic, 22-bit operands, fp32 accumulate: ~3 x torch's fp32 GEMM at these sizes
    and closer to float64); the weight's pieces are made once.  Small products and everything else stay with torch.

matmul_nbits, counted per MatMulNBits node in `nbits_calls`:
    "fused": a node the library has a kernel for (`ops.matmul_nbits`: integer zero points, a block size that is a multiple of 32,
        4 / 8 bits, a constant B) runs from the blob as stored -- no [N, K] weight is expanded.
    "fused+decode": a node whose flattened A has at most 16 rows and which the decode kernel takes (`ops.matmul_nbits_decode`: also
        float zero points -- HQQ files -- and block size 16) runs there, counted as "decode"; every other node as under "fused".
    "fused+float_zp" / "fused+float_zp+decode": as "fused" / "fused+decode", and a node with floating-point zero points and a block
        size that is a multiple of 32 which those leave runs on `ops.matmul_nbits_float_zp`, counted as "float_zp".

qlinear, counted per QLinearMatMul / QGemm node in `qlinear_calls` and per function call in `qlinear_function_calls`:
    "fused": a node the library has a kernel for (`ops.qlinear_matmul`: 8-bit operands, per-tensor activation parameters, fp32
        scales, a constant 2-D B, alpha = 1, no transA) runs on the int8 matrix cores, an exact int32 sum; nothing is dequantized.
    "fused+decode": such a node whose flattened A has at most 16 rows runs on `ops.qlinear_matmul_decode` (B streamed once, the same
        accumulator and epilogue, so the same bytes), counted as "decode"; every other node as under "fused".
    "function": a call of a `quant`-domain function QLinearMatMul / QLinearGemm (what a `format="qlinear"` file holds) whose body is
        the one `onnx_functions.build_function` writes -- QuantizeLinear, the integer product, DequantizeLinear -- runs as ONE library
        call (`ops.qlinear_function`: fp32 in, fp32 out, the bytes of the three nodes) when W and every parameter are held.  Every
        other call walks its body ("body"), whose integer node then goes as under "fused".
    "function+decode": such a call with at most 16 flattened rows runs on `ops.qlinear_function_decode` ("decode"); everything else
        as under "function", the body's integer node as under "fused+decode".

qdq, counted per call of a `quant`-domain QDQ function (the default output format) in `qdq_calls`, or, for the calls the integer
routes are asked about, in `qdq_function_calls`.  Which kernel takes a call follows from how its W is held, not from an order:
    "fused": a call whose body is the one `build_function` writes runs its product from the stored integers (`ops.qdq_matmul`:
        W [K, N] bytes, its scales and zero points as the file holds them; no fp32 weight is made).  The body's own operators around
        the product -- Q -> DQ of the input, of the output, DQ of the bias -- run as they are.  Every other call walks the body ("torch").
    "fused+integer": as "fused", and a call of a function with an input Q -> DQ (static or dynamic; with or without an output
        Q -> DQ) runs as ONE library call (`ops.qdq_function`: fp32 in, fp32 out, the product of the 8-bit activations and the stored
        W as an exact int32 sum on the int8 matrix cores) when W, its parameters, the static activation parameters and the bias
        triple are held and X is a non-empty fp32 tensor: "integer", or "body" where a condition fails.
    "fused+packed4": as "fused", and an INT4 / UINT4 initializer [K, N] with an even N that nothing reads but recognised QDQ
        functions, as their W, is uploaded as the file's packed bytes -- uint8 [K, N / 2], two values a byte -- and never held
        unpacked: half the HBM, the upload and the weight read.  Its calls run on `ops.qdq_matmul_packed4` ("packed4"); a call the
        kernel leaves out unpacks W on the device for that call and walks the body ("torch").
    "fused+integer+packed4": the two combined.  A call of a function with an input Q -> DQ whose W is held packed runs as one call of
        `ops.qdq_function_packed4` ("packed4"); a 4-bit W that is not held packed (an odd N), or a call the packed kernel leaves
        out, walks the body ("body") -- no unpacked 4-bit W feeds the 8-bit kernel in this mode.
    "fused+integer+packed4+decode": as "fused+integer+packed4", and a call that would run on `ops.qdq_function_packed4` and whose
        flattened X has at most 16 rows runs on `ops.qdq_function_packed4_decode` instead (the nibbles streamed once, the same
        bytes), counted as "decode".
    "fused+integer+decode": as "fused+integer", and a call that would run on `ops.qdq_function` and whose flattened X has at most 16
        rows runs on `ops.qdq_function_decode` instead (the [K, N] bytes streamed once, the same bytes), counted as
        "integer_decode".
    "fused+integer+decode+packed4": "fused+integer+packed4+decode" and "fused+integer+decode" combined: a W held packed goes as
        under the first, every other W as under the second.
"""
from __future__ import annotations

import torch

from .onnx_functions import _QDQ, QUANT_DOMAIN, build_function
from .onnx_proto import DataType, attribute_value

# keyword value -> the routes it tries, in order (the docstring says what each is)
NBITS_MODES = {"torch": (), "fused": ("fused",), "fused+decode": ("decode", "fused"), "fused+float_zp": ("fused", "float_zp"),
               "fused+float_zp+decode": ("decode", "fused", "float_zp")}
# ... -> (the routes of a bare QLinearMatMul / QGemm node, the routes of a call of a QLinear function)
QLINEAR_MODES = {"torch": ((), ()), "fused": (("fused",), ()), "fused+decode": (("decode", "fused"), ()), "function": (("fused",), ("function",)),
                 "function+decode": (("decode", "fused"), ("decode", "function"))}
# ... -> (the routes of a QDQ function's product, the routes of a whole call of one with an input Q -> DQ)
QDQ_MODES = {"torch": ((), ()), "fused": (("fused",), ()), "fused+integer": (("fused",), ("integer",)), "fused+packed4": (("fused", "packed4"), ()),
             "fused+integer+packed4": (("fused", "packed4"), ("integer", "packed4")),
             "fused+integer+packed4+decode": (("fused", "packed4"), ("integer", "packed4", "decode")),
             "fused+integer+decode": (("fused",), ("integer", "integer_decode")),
             "fused+integer+decode+packed4": (("fused", "packed4"), ("integer", "integer_decode", "packed4", "decode"))}
MATMUL_MODES = {"torch": False, "pieces": True}

# route -> the `ops` function that runs it; `<that name>_unsupported` says what the kernel leaves out
_KERNELS = {"nbits": {"decode": "matmul_nbits_decode", "fused": "matmul_nbits", "float_zp": "matmul_nbits_float_zp"},
            "qlinear": {"decode": "qlinear_matmul_decode", "fused": "qlinear_matmul"},
            "qlinear_function": {"decode": "qlinear_function_decode", "function": "qlinear_function"},
            "qdq": {"packed4": "qdq_matmul_packed4", "fused": "qdq_matmul"},
            "qdq_function": {"decode": "qdq_function_packed4_decode", "packed4": "qdq_function_packed4", "integer_decode": "qdq_function_decode",
                             "integer": "qdq_function"}}

_PIECES_MIN_WIDTH, _PIECES_MIN_ROWS = 512, 256


def _kernel(what: str, route: str):
    """(the `ops` function of a route, its `_unsupported`).  The library is loaded by the first route that asks."""
    from .hip import ops
    name = _KERNELS[what][route]
    return getattr(ops, name), getattr(ops, name + "_unsupported")


def accepted_mode(keyword: str, table, value: str) -> str:
    if value not in table:
        names = [repr(m) for m in table]
        raise ValueError(f"GraphRunner: {keyword} must be {', '.join(names[:-1])} or {names[-1]}, got {value!r}")
    return value


def counter(base, routes) -> dict:
    """A call counter: the keys every mode has, then the ones only this mode's routes add."""
    return dict.fromkeys(tuple(base) + tuple(r for r in routes if r not in base), 0)


def first_route(routes, accepts, otherwise: str) -> str:
    return next((r for r in routes if accepts(r)), otherwise)


def _ints(t) -> list[int]:
    """A shape-like operand as Python ints (one sync when it lives on the device; shape arithmetic is kept on the host)."""
    return [int(v) for v in (t.tolist() if t.ndim else [t.item()])]


class ById(dict):
    """A table keyed by what an object IS: id(object) -> (the object, its value).  The object is kept next to its value, so its id
    cannot pass to another object while the entry stands; every hit is checked with `is` all the same."""

    def value(self, obj, default=None):
        hit = self.get(id(obj))
        return hit[1] if hit is not None and hit[0] is obj else default

    def memo(self, obj, make):
        hit = self.get(id(obj))
        if hit is None or hit[0] is not obj:
            hit = self[id(obj)] = (obj, make(obj))
        return hit[1]


def _unpacked4(w, held):
    """A weight held as packed nibbles [K, N / 2] (``held``: its `_packed4` entry) as one value per byte [K, N], on the device."""
    n, signed = held
    q = torch.stack((w & 0x0F, w >> 4), dim=-1).reshape(w.shape[0], n)
    return ((q ^ 8).to(torch.int8) - 8) if signed else q


def _qlinear_function_named(fn) -> bool:
    """`fn` carries the name of a QLinear function of the `quant` domain (onnx_functions._qlinear_function)."""
    return (fn.domain or "") == QUANT_DOMAIN and fn.name in ("QLinearMatMul", "QLinearGemm")


class _QdqPlan:
    """How a `quant`-domain QDQ function (onnx_functions.py) is run with its product fused: which nodes of the body dequantize W
    (left out), which one is the product (replaced), and what the product reads."""
    _GROUPED = ("QMatMulWeightsOnlyGrouped", "QGemmWeightsOnlyGrouped")

    def __init__(self, weight_nodes, product, x, bias, group_size):
        self.weight_nodes, self.product, self.x, self.bias, self.group_size = weight_nodes, product, x, bias, group_size

    @staticmethod
    def _shape(fn):
        """What is compared: inputs, outputs, and per node its operator, domain, wiring and attributes."""
        return (list(fn.input), list(fn.output),
                [(n.op_type, n.domain or "", list(n.input), list(n.output), sorted((a.name, repr(attribute_value(a))) for a in n.attribute))
                 for n in fn.node])

    @classmethod
    def named(cls, fn) -> bool:
        """`fn` carries the name of a QDQ function of the `quant` domain."""
        return (fn.domain or "") == QUANT_DOMAIN and (fn.name in _QDQ or fn.name in cls._GROUPED)

    @staticmethod
    def input_mode(fn):
        """`fn` carries the name of a QDQ function with an input Q -> DQ: "static" / "dynamic", else None."""
        return _QDQ[fn.name][1][0] if (fn.domain or "") == QUANT_DOMAIN and fn.name in _QDQ else None

    @classmethod
    def of(cls, fn):
        if not cls.named(fn):
            return None
        nodes = list(fn.node)
        if fn.name in _QDQ:
            expected, group_size = build_function(fn.name), 0
        else:
            blocked = [n for n in nodes if n.op_type == "DequantizeLinear" and any(a.name == "block_size" for a in n.attribute)]
            if len(blocked) != 1:
                return None
            group_size = int(attribute_value(next(a for a in blocked[0].attribute if a.name == "block_size")))
            if group_size <= 0:
                return None
            expected = build_function(fn.name, group_size=group_size, four_bit=bool(nodes) and nodes[0].op_type == "Cast")
        if cls._shape(fn) != cls._shape(expected):
            return None
        product = next(i for i, n in enumerate(nodes) if n.op_type in ("MatMul", "Gemm"))
        node = nodes[product]
        # the nodes between W and `dequantized_weights`: everything the product's second operand depends on
        needed, weight_nodes = {node.input[1]}, set()
        for i in range(product - 1, -1, -1):
            if any(o in needed for o in nodes[i].output):
                weight_nodes.add(i)
                needed.update(name for name in nodes[i].input if name)
        return cls(weight_nodes, product, node.input[0], node.input[2] if len(node.input) > 2 else None, group_size)


class Routes:
    """What `GraphRunner` inherits to route with.  It reads the runner's `device`, `graph`, `functions`, `wanted` and `constants` and
    calls its `_reads` and `_run`."""
    _unpacked4 = staticmethod(_unpacked4)

    def _init_routes(self, matmul: str, matmul_nbits: str, qlinear: str, qdq: str):
        """The mode attributes, the route tuples behind them, the counters and the caches (before the constants are uploaded)."""
        modes = (accepted_mode("matmul", MATMUL_MODES, matmul), accepted_mode("matmul_nbits", NBITS_MODES, matmul_nbits),
                 accepted_mode("qlinear", QLINEAR_MODES, qlinear), accepted_mode("qdq", QDQ_MODES, qdq))
        self.matmul, self.matmul_nbits, self.qlinear, self.qdq = modes if self.device.type == "cuda" else ("torch",) * 4
        self._pieces = MATMUL_MODES[self.matmul]
        self._nbits_routes = NBITS_MODES[self.matmul_nbits]
        self._qlinear_routes, self._qlinear_function_routes = QLINEAR_MODES[self.qlinear]
        self._qdq_routes, self._qdq_function_routes = QDQ_MODES[self.qdq]
        self.nbits_calls = counter(("fused", "torch"), self._nbits_routes)
        self.qlinear_calls = counter(("fused", "torch"), self._qlinear_routes)
        self.qlinear_function_calls = counter(("function", "body"), self._qlinear_function_routes)
        self.qdq_calls = counter(("fused", "torch"), self._qdq_routes)
        self.qdq_function_calls = counter(("integer", "body"), self._qdq_function_routes)
        self._weight_pieces = ById()         # constant weight -> its MatmulOperand (None: HBM had no room for the pieces)
        self._written = ById()               # function -> its _QdqPlan (QDQ) / True (QLinear) where its body is the writer's, else None
        self._qdq_bias = ById()              # constant B or b_zero_point -> its int32 copy
        # how a 4-bit constant is held where "packed4" is on: (N, its nibbles are signed) for packed nibbles [K, N / 2], () for one value per byte
        self._packed4 = ById()

    def _held(self, t) -> bool:
        """`t` is a tensor on the runner's device and is, by identity, a constant of the model."""
        return isinstance(t, torch.Tensor) and t.device.type == self.device.type and self._constant_ids.value(t, False)

    # ---------------------------------------------------------------------------------------------- 4-bit weights held packed
    def _packable_weights(self) -> set:
        """The names of the INT4 / UINT4 initializers "packed4" holds packed: two axes, an even N, no external data, not a wanted
        value, and every reader in the graph a call of a recognised QDQ function with the initializer as its W and nothing else."""
        four_bit = {t.name for t in self.graph.initializer if t.data_type in (DataType.INT4, DataType.UINT4) and len(t.dims) == 2
                    and int(t.dims[1]) % 2 == 0 and int(t.dims[0]) > 0 and int(t.dims[1]) > 0 and not t.data_location}
        four_bit -= set(self.wanted) | {o.name for o in self.graph.output}
        read = set()
        for node in self.graph.node:
            fn = self.functions.get((node.domain or "", node.op_type, node.overload or ""))
            as_w = fn is not None and _QdqPlan.named(fn) and self._writers(fn) is not None and "W" in fn.input
            inputs = list(node.input)
            for name in self._reads(node):
                if name in four_bit and not (as_w and inputs.count(name) == 1 and inputs.index(name) == list(fn.input).index("W")):
                    four_bit.discard(name)
                read.add(name)
        return four_bit & read

    def _as_int32(self, t):
        """A constant of the bias triple as the library call takes it.  The writer stores B and its zero point in the weight's 8-bit
        type; the same integers as int32, made once per constant."""
        if t is None or t.dtype not in (torch.int8, torch.uint8):
            return t
        return self._qdq_bias.memo(t, lambda t: t.to(torch.int32))

    # ---------------------------------------------------------------------------------------------- function calls
    def _writers(self, fn):
        """What runs a `quant`-domain function whose body is the one `onnx_functions.build_function` writes under its name: its
        `_QdqPlan` (a QDQ function) or True (a QLinear function); None for every other function -- a file may carry another
        function under a reference name."""
        return self._written.memo(fn, lambda fn: _QdqPlan.of(fn) if not _qlinear_function_named(fn) else
                                  _QdqPlan._shape(fn) == _QdqPlan._shape(build_function(fn.name)) or None)

    def _route_call(self, fn, env):
        """A call of a function of the model, with its inputs in `env`: the outputs where a route ran it; None where the body is to
        be walked on `env`.  Counted per call, under the key the outcome names."""
        if _QdqPlan.named(fn):
            if self._qdq_function_routes and _QdqPlan.input_mode(fn) is not None:
                calls, (key, outs) = self.qdq_function_calls, self._run_qdq_function(fn, env)
            else:
                calls, (key, outs) = self.qdq_calls, self._run_qdq_fused(fn, env)
        elif self._qlinear_function_routes and _qlinear_function_named(fn):
            calls, (key, outs) = self.qlinear_function_calls, self._run_qlinear_function(fn, env)
        else:
            return None
        calls[key] += 1
        packed = self._packed4.value(env.get("W"))
        if outs is None and packed:            # what the kernel leaves out: the body reads W one value per byte, for this call only
            env["W"] = _unpacked4(env["W"], packed)
        return outs

    def _one_call(self, fn, env, names) -> bool:
        """What every one-call route asks first: the body is the writer's, X is a non-empty fp32 tensor on the GPU, and each of the
        named inputs is absent or held."""
        if self._writers(fn) is None:
            return False
        x = env["X"]
        return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim >= 1
                and x.numel() > 0 and all(env[n] is None or self._held(env[n]) for n in names))

    def _run_qlinear_function(self, fn, env):
        """One call of a `quant`-domain QLinearMatMul / QLinearGemm function as one library call: (route, the function's outputs), or
        ("body", None) -- nothing was run -- where `_one_call` refuses or the kernels have no route for the call."""
        gemm = fn.name == "QLinearGemm"
        if not self._one_call(fn, env, ("W", "w_scale", "w_zero_point", "x_scale", "x_zero_point", "out_scale", "out_zero_point") + (("B",) if gemm else ())):
            return "body", None
        args = (env["X"], env["x_scale"], env["x_zero_point"], env["W"], env["w_scale"], env["w_zero_point"], env["out_scale"], env["out_zero_point"])
        bias = env.get("B") if gemm else None
        route = first_route(self._qlinear_function_routes, lambda r: _kernel("qlinear_function", r)[1](*args, bias=bias) is None, "body")
        return route, None if route == "body" else (_kernel("qlinear_function", route)[0](*args, bias=bias),)

    def _run_qdq_function(self, fn, env):
        """One call of a QDQ function with an input Q -> DQ as one library call (`ops.qdq_function`; `ops.qdq_function_packed4` where
        W is held as packed nibbles; `ops.qdq_function_decode` / `ops.qdq_function_packed4_decode` in their places where the mode
        has them and they take the call): (route, the function's outputs), or ("body", None) -- nothing was run -- where `_one_call`
        refuses, W, its scale or B is absent, or the kernel has no route for the call."""
        op, (x_mode, out_mode) = _QDQ[fn.name]
        names = ["W", "w_scale", "w_zero_point"] + (["B", "b_scale", "b_zero_point"] if op == "Gemm" else []) + \
            (["x_scale", "x_zero_point"] if x_mode == "static" else []) + (["out_scale", "out_zero_point"] if out_mode == "static" else [])
        if not self._one_call(fn, env, names) or env["W"] is None or env["w_scale"] is None or (op == "Gemm" and env["B"] is None):
            return "body", None
        x_scale, x_zero_point = (env.get("x_scale"), env.get("x_zero_point")) if x_mode == "static" else (None, None)
        out_scale, out_zero_point = (env.get("out_scale"), env.get("out_zero_point")) if out_mode == "static" else (None, None)
        args = dict(x_mode=x_mode, x_scale=x_scale, x_zero_point=x_zero_point, out_mode=out_mode, out_scale=out_scale, out_zero_point=out_zero_point,
                    bias=(self._as_int32(env["B"]), env["b_scale"], self._as_int32(env["b_zero_point"])) if op == "Gemm" else None)
        w, held = env["W"], self._packed4.value(env["W"])
        if held == ():                         # a 4-bit W this mode could not hold packed: no unpacked copy feeds the 8-bit kernel
            return "body", None
        routes = tuple(r for r in ("integer_decode", "integer") if r in self._qdq_function_routes)
        if held:                               # the decode kernels first where the mode has them: they refuse more than 16 rows by themselves
            routes, (args["n"], args["signed"]) = tuple(r for r in ("decode", "packed4") if r in self._qdq_function_routes), held
        operands = (env["X"], w, env["w_scale"], env["w_zero_point"])
        route = first_route(routes, lambda r: _kernel("qdq_function", r)[1](*operands, **args) is None, "body")
        return route, None if route == "body" else (_kernel("qdq_function", route)[0](*operands, **args),)

    def _run_qdq_fused(self, fn, env):
        """One call of a recognised QDQ function with its product on `ops.qdq_matmul` -- on `ops.qdq_matmul_packed4` where W is held
        as packed nibbles: the nodes of the body that dequantize W are left out, the product node is replaced, every other node runs
        as it is, on a copy of `env`.  (route, the function's outputs), or ("torch", None) -- nothing is kept -- where the mode is "torch", the
        body is not the writer's or the kernel has no route for the call: the whole body then runs."""
        plan = self._writers(fn) if self._qdq_routes else None
        if plan is None:
            return "torch", None
        env = dict(env)
        w, scale, zp = env["W"], env["w_scale"], env["w_zero_point"]
        if not all(self._held(t) for t in (w, scale) + (() if zp is None else (zp,))):
            return "torch", None
        args, route = dict(group_size=plan.group_size), "fused"
        packed = self._packed4.value(w)
        if packed:
            route, (args["n"], args["signed"]) = "packed4", packed
        if w.ndim != 2:
            return "torch", None
        if plan.group_size:
            shape = env.get("original_transposed_shape")
            if not isinstance(shape, torch.Tensor) or shape.is_cuda or _ints(shape) != [args.get("n", w.shape[1]), w.shape[0]]:
                return "torch", None
        nodes = list(fn.node)
        self._run([n for i, n in enumerate(nodes[:plan.product]) if i not in plan.weight_nodes], env)      # the input side, the bias
        x, args["bias"] = env[plan.x], env[plan.bias] if plan.bias else None
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.numel() > 0 and (args["bias"] is None or (isinstance(args["bias"], torch.Tensor) and args["bias"].is_cuda))):
            return "torch", None
        run, unsupported = _kernel("qdq", route)
        if unsupported(x, w, scale, zp, **args) is not None:
            return "torch", None
        env[nodes[plan.product].output[0]] = run(x, w, scale, zp, **args)
        self._run(nodes[plan.product + 1:], env)                                                            # the output side
        return route, tuple(env[o] for o in fn.output)

    # ---------------------------------------------------------------------------------------------- nodes
    def _run_nbits(self, x, K, N, bits, g):
        """A MatMulNBits node on the first route of the mode that takes it, counted: its output, or None for the torch expansion."""
        route = first_route(self._nbits_routes, lambda r: self._nbits_fusable(r, x, bits, g), "torch")
        self.nbits_calls[route] += 1
        if route == "torch":
            return None
        return _kernel("nbits", route)[0](*x[:3], x[3] if len(x) > 3 else None, K=K, N=N, bits=bits, block_size=g, bias=x[5] if len(x) > 5 else None)

    def _nbits_fusable(self, route, x, bits, g) -> bool:
        """Whether the kernel of ``route`` -- "fused": `ops.matmul_nbits`; "decode": `ops.matmul_nbits_decode`, which also wants at
        most 16 rows of A; "float_zp": `ops.matmul_nbits_float_zp`, which wants floating-point zero points -- takes this MatMulNBits
        node: what the kernel supports, on the GPU, with B, scales and zero points held as the writer stores them."""
        zp, g_idx, bias = (list(x[3:6]) + [None] * 3)[:3]
        if not (isinstance(x[0], torch.Tensor) and x[0].is_cuda and x[0].ndim >= 1 and x[0].numel() > 0):
            return False
        rows = dict(rows=x[0].numel() // x[0].shape[-1] if x[0].shape[-1] else 0) if route == "decode" else {}
        if _kernel("nbits", route)[1](x[0].dtype, bits, g, zp, g_idx, **rows) is not None:
            return False
        if not all(t is None or self._held(t) for t in (x[1], x[2], zp)):
            return False
        zp_types = {"decode": (torch.uint8, torch.float32, x[0].dtype), "float_zp": (torch.float32, x[0].dtype), "fused": (torch.uint8,)}[route]
        return (x[1].dtype == torch.uint8 and x[2].dtype in (torch.float32, x[0].dtype) and (zp is None or zp.dtype in zp_types)
                and (bias is None or (bias.is_cuda and bias.dtype == x[0].dtype)))

    def _run_qlinear(self, A, a_scale, a_zp, B, b_scale, b_zp, y_scale, y_zp, bias=None, trans_b=False, alpha=1.0, trans_a=False):
        """A QLinearMatMul / QGemm node on the first route of the mode that takes it, counted: its output, or None (torch)."""
        operands = (A, a_scale, a_zp, B, b_scale, b_zp, y_scale, y_zp)
        route = first_route(self._qlinear_routes, lambda r: self._qlinear_fusable(r, *operands, bias, trans_b, alpha, trans_a), "torch")
        self.qlinear_calls[route] += 1
        return None if route == "torch" else _kernel("qlinear", route)[0](*operands, bias=bias, trans_b=trans_b)

    def _qlinear_fusable(self, route, A, a_scale, a_zp, B, b_scale, b_zp, y_scale, y_zp, bias, trans_b, alpha, trans_a) -> bool:
        """Whether the kernel of ``route`` -- "fused": `ops.qlinear_matmul`; "decode": `ops.qlinear_matmul_decode`, which also wants
        at most 16 rows of A -- takes this QLinearMatMul / QGemm node: A an 8-bit tensor on the GPU, every parameter a tensor on the
        GPU, B, its parameters and C held, and nothing the kernel leaves out."""
        if not (isinstance(A, torch.Tensor) and A.is_cuda and A.dtype in (torch.uint8, torch.int8) and A.ndim >= 1 and A.numel() > 0):
            return False
        every = (a_scale, a_zp, B, b_scale, b_zp, y_scale, y_zp, bias)
        if a_scale is None or B is None or b_scale is None or not all(t is None or (isinstance(t, torch.Tensor) and t.is_cuda) for t in every):
            return False
        if not all(t is None or self._held(t) for t in (B, b_scale, b_zp, bias)):
            return False
        return _kernel("qlinear", route)[1](A, a_scale, a_zp, B, b_scale, b_zp, y_scale, y_zp, bias=bias, trans_b=trans_b, alpha=alpha, trans_a=trans_a) is None

    def _run_pieces(self, x, w, headroom):
        """A MatMul of fp32 activations with a large held weight on `ops.matmul_pieces`: its output, or None for torch's GEMM."""
        if not (self._pieces and w.ndim == 2 and w.dtype == torch.float32 and x.dtype == torch.float32 and x.is_cuda and min(w.shape) >= _PIECES_MIN_WIDTH
                and x.numel() // max(1, w.shape[0]) >= _PIECES_MIN_ROWS and x.ndim >= 2 and self._held(w)):
            return None
        from .hip import ops

        def pieces(w):
            # the pieces are a second copy of the weight (two fp16 halves): kept only while HBM has room for them and the
            # activations of a pass; past that the product stays with torch's fp32 GEMM on the weight itself
            free = torch.cuda.mem_get_info(w.device)[0] + torch.cuda.memory_reserved(w.device) - torch.cuda.memory_allocated(w.device)
            return ops.matmul_prepare(w, False) if free > headroom * w.numel() * 4 else None
        operand = self._weight_pieces.memo(w, pieces)
        return None if operand is None else ops.matmul_pieces(x, operand)
