"""HQQ (reference core/_algorithms/hqq.py).

CPU: the oracle's restatement against golden vectors produced by the reference's own `_hqq_quantize`
(tests/golden/make_golden.py::gen_hqq) -- bit for bit -- and the reference's configuration rules
(test/core/test_qconfig.py:315-395).  GPU (`-m gpu`): oq_hqq_optimize_f32 against the oracle.

The GPU contract:
  * lp_norm = 1: the oracle's BITS -- scales, zero points, integers, blob and round count.  The shrink's power is x^0 = 1 on
    both sides, every other step of a round is one correctly rounded fp32 operation, and the row means follow NumPy's pairwise
    summation tree.  tests/test_hqq_exact_gpu.py holds that on every route, block edge and group size; here the golden case c4
    (lp_norm = 1; tests/test_hqq_cases.py asserts that its trace meets the decision condition) is compared byte for byte.
  * any lp_norm: the integers are exact GIVEN the zero points the kernel returned, q == clip(round(w / s + z_kernel)): the
    finish kernel's arithmetic is IEEE.  A differing integer can therefore come only from a differing zero point.
  * lp_norm != 1: np.power (fp32) is not bit-reproducible on a GPU.  The zero point update is a contraction-free
    fixed-point iteration, so a last-bit difference stays a last-bit difference: zero points agree to 2e-5 absolute (values
    live in [0, 15]), scales are bit-equal (same RTN kernel), and an integer may differ only where w / scale + zero_point is
    within that distance of a rounding tie -- bounded here by 0.1 % of the elements and never by more than one level.
"""
import numpy as np
import pytest

import oq_oracle as O
from hqq_cases import integers_given
from conftest import load_json, load_npz, synth_weight
from onnx_quantize_amd import HqqConfig, QConfig, QuantizationStrategy, QuantType, QWeightArgs

CASES = load_json("hqq.json")["cases"]
GOLD = load_npz("hqq.npz")


def _args(c):
    return (c["group_size"], c["reduce_range"], c["clip_ratio"], c["mse"], c["lp_norm"], c["beta"], c["kappa"], c["iters"],
            c["early_stop"])


@pytest.mark.parametrize("case", CASES, ids=[c["key"] for c in CASES])
def test_oracle_reproduces_reference_bit_for_bit(case):
    w = synth_weight(case["kind"], case["seed"], case["k"], case["n"])
    q, s, z = O.hqq_quantize(w, *_args(case))
    k = case["key"]
    assert np.array_equal(q, GOLD[k + "_q"])
    assert s.tobytes() == GOLD[k + "_s"].tobytes() and z.tobytes() == GOLD[k + "_z"].tobytes()
    assert s.dtype == np.float32 and z.dtype == np.float32 and z.shape == s.shape == (case["k"] * case["n"] // _g(case), 1)


def _g(c):
    return c["k"] if c["group_size"] in (-1,) or c["group_size"] > c["k"] else c["group_size"]


def test_reference_property_reconstruction_within_half_level(rng):
    """test/core/algorithms/test_hqq.py:10-36: |W - dequant| <= 0.5 on the reference's own input."""
    w = rng.standard_normal((32, 64)).astype(np.float32)
    for g in (16, 32):
        q, s, z = O.hqq_quantize(w, g)
        rows = O.to_rows(q, "group", g).astype(np.float32)
        wr = O.from_rows((rows - z) * s, w, "group")
        np.testing.assert_allclose(w, wr, atol=5e-1)


class TestHqqConfig:
    def test_valid(self):
        a = QWeightArgs(dtype=QuantType.QUInt4, strategy=QuantizationStrategy.GROUP, group_size=32, symmetric=False,
                        algorithm=HqqConfig())
        assert isinstance(a.algorithm, HqqConfig) and a.zp_dtype == a.scale_dtype and a.group_size == 32

    def test_defaults_and_registry(self):
        c = HqqConfig()
        assert (c.algorithm_type, c.lp_norm, c.beta, c.kappa, c.iters, c.early_stop) == ("hqq", 0.7, 10.0, 1.01, 20, True)
        a = QWeightArgs(dtype="uint4", strategy="group", group_size=64, algorithm={"algorithm_type": "hqq", "iters": 5})
        assert isinstance(a.algorithm, HqqConfig) and a.algorithm.iters == 5
        q = QConfig(weights=a)
        assert QConfig(**q.model_dump()).weights.algorithm.iters == 5       # survives the per-node round trip

    @pytest.mark.parametrize("qt", [QuantType.QInt8, QuantType.QUInt8])
    def test_invalid_dtype(self, qt):
        with pytest.raises(ValueError, match="HQQ only supports uint4 weight type"):
            QWeightArgs(dtype=qt, strategy="group", group_size=32, algorithm=HqqConfig())

    def test_invalid_symmetric(self):
        with pytest.raises(ValueError, match="HQQ only supports asymmetric quantization"):
            QWeightArgs(dtype="uint4", strategy="group", group_size=32, symmetric=True, algorithm=HqqConfig())

    @pytest.mark.parametrize("strategy", ["tensor", "channel"])
    def test_invalid_strategy(self, strategy):
        with pytest.raises(ValueError, match="HQQ only supports 'group' quantization strategy"):
            QWeightArgs(dtype="uint4", strategy=strategy, algorithm=HqqConfig())

    @pytest.mark.parametrize("g", [8, 48])
    def test_invalid_group_size(self, g):
        with pytest.raises(ValueError, match="HQQ requires group_size to be greater than 16"):
            QWeightArgs(dtype="uint4", strategy="group", group_size=g, algorithm=HqqConfig())

    def test_valid_group_sizes(self):
        for g in (16, 32, 64, 128, 256):
            assert QWeightArgs(dtype="uint4", strategy="group", group_size=g, algorithm=HqqConfig()).group_size == g


# ------------------------------------------------------------------------------------------------ GPU
def _check_against_oracle(w, q, s, z, eq, es, ez, label, group_size, reduce_range=False, exact=False):
    assert s.tobytes() == es.tobytes(), f"{label}: scales differ"
    assert q.tobytes() == integers_given(w, s, z, group_size, reduce_range).tobytes(), f"{label}: q is not clip(round(w / s + z)) of the returned z"
    if exact:
        assert z.tobytes() == ez.tobytes() and q.tobytes() == eq.tobytes(), f"{label}: lp_norm = 1 owes the oracle's bits"
    assert z.shape == ez.shape and z.dtype == np.float32
    dz = np.abs(z - ez).max()
    assert dz <= 2e-5, f"{label}: zero points differ by {dz}"
    diff = q.astype(np.int16) - eq.astype(np.int16)
    assert np.abs(diff).max() <= 1, f"{label}: an integer moved by more than one level"
    frac = np.count_nonzero(diff) / diff.size
    assert frac <= 1e-3, f"{label}: {frac:.2%} of the integers differ"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["key"] for c in CASES])
def test_gpu_matches_golden(case):
    import torch
    from onnx_quantize_amd.hip import ops
    w = synth_weight(case["kind"], case["seed"], case["k"], case["n"])
    q, s, z, rounds = ops.hqq_quantize(torch.from_numpy(w).cuda(), *_args(case))
    k = case["key"]
    _check_against_oracle(w, q.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy(), GOLD[k + "_q"], GOLD[k + "_s"], GOLD[k + "_z"], k,
                          case["group_size"], case["reduce_range"], exact=case["lp_norm"] == 1.0)
    assert 1 <= int(rounds.item()) <= case["iters"]


@pytest.mark.gpu
def test_gpu_rounds_and_early_stop_follow_the_oracle():
    """Same number of evaluated rounds as the reference loop (the device-side decision), with and without early stop."""
    import torch
    from onnx_quantize_amd.hip import ops
    w = np.random.default_rng(5).standard_normal((256, 192), dtype=np.float32)
    for early in (True, False):
        rows = O.to_rows(w, "group", 64)
        s, z0 = O.qparams_from_rows(rows, "uint4", "group", False, False, 1.0, False, np.float32, np.float32)
        trace = []
        O.hqq_optimize_zero_point(rows, s, z0, False, 0.7, 10.0, 1.01, 20, early, trace=trace)
        _, _, _, rounds = ops.hqq_quantize(torch.from_numpy(w).cuda(), 64, early_stop=early)
        assert int(rounds.item()) == len(trace)


@pytest.mark.gpu
def test_gpu_plugin_seam_and_medium_matrix():
    """HqqConfig.quantize_weights-equivalent functional mirror on a 1024 x 1536 matrix, g = 128 (MatMulNBits shape)."""
    from onnx_quantize_amd.algorithms import _hqq_quantize
    w = np.random.default_rng(9).standard_normal((1024, 1536), dtype=np.float32)
    q, s, z = _hqq_quantize(w, QuantType.QUInt4, 128)
    eq, es, ez = O.hqq_quantize(w, 128)
    assert q.shape == w.shape and s.shape == z.shape == (1024 * 1536 // 128, 1) and z.dtype == s.dtype == np.float32
    _check_against_oracle(w, q.astype(np.uint8), s, z, eq, es, ez, "1024x1536", 128)
    # the optimisation does what it is for: lower mean |W - dequant| than plain RTN (hqq.py:131)
    rq, rs, rz = O.rtn_quantize(w, "uint4", "group", 128)
    err = lambda qq, ss, zz: np.abs(O.to_rows(w, "group", 128) - (O.to_rows(qq, "group", 128).astype(np.float32) - zz) * ss).mean()  # noqa: E731
    assert err(q.astype(np.uint8), s, z) < err(rq, rs, rz.astype(np.float32))


@pytest.mark.gpu
def test_gpu_matmul_nbits_blob_equals_packed_kn_result():
    """layout="nbits": the blob HQQ's only consumer (MatMulNBits) takes, qrules/_common.py:65-99 -- the same integers as
    the [K, N] result, packed two per byte along k; float zero points stay one per group."""
    import torch
    from onnx_quantize_amd.hip import ops
    w = torch.from_numpy(np.random.default_rng(12).standard_normal((512, 200), dtype=np.float32)).cuda()
    for g in (16, 64, 128):
        q, s, z, _ = ops.hqq_quantize(w, g)
        b, s2, z2, _ = ops.hqq_quantize(w, g, layout="nbits")
        eb, es, ez = O.matmul_nbits_layout(q.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy(), g, 4, zp_is_float=True)
        np.testing.assert_array_equal(b.cpu().numpy(), eb)
        assert torch.equal(s, s2) and torch.equal(z, z2) and ez.shape == (200, 512 // g) and ez.dtype == np.float32


@pytest.mark.gpu
def test_gpu_errors_are_loud():
    import torch
    from onnx_quantize_amd.hip import ops
    with pytest.raises(TypeError):
        ops.hqq_quantize(torch.zeros((64, 64)), 32)
    with pytest.raises(ValueError, match="cannot reshape"):
        ops.hqq_quantize(torch.zeros((10, 3), device="cuda"), 4)


@pytest.mark.gpu
@pytest.mark.parametrize("g", [16, 32, 64, 128])
def test_gpu_one_pass_route_gives_the_per_round_route_s_bits(g):
    """all rounds of a row out of registers in one pass over W (hqq_rounds_reg_kernel + the replayed
    decisions) against one launch pair per round (W re-read every round): the same zero points, integers and round counts,
    bit for bit -- with and without early stop, with an early stop that really triggers (a huge kappa makes the error rise
    after a few rounds), ragged columns, a leading dimension, and the blob layout."""
    import torch
    from onnx_quantize_amd.hip import ops
    gen = torch.Generator(device="cuda").manual_seed(40 + g)
    big = torch.randn((512, 600), generator=gen, device="cuda") * (0.5 + torch.rand(600, generator=gen, device="cuda"))
    for w in (big[:, :520], big[:256, 8:8 + 132]):            # ldw = 600; N % 256 != 0, N % 4 == 0 / != 0 mixes
        for kwargs in (dict(), dict(early_stop=False, iters=9), dict(kappa=3.0, iters=12), dict(iters=1), dict(reduce_range=True)):
            a = ops.hqq_quantize(w, g, **kwargs)
            b = ops.hqq_quantize(w, g, per_round_launches=True, **kwargs)
            assert int(a[3]) == int(b[3]) >= 1, (g, kwargs, int(a[3]), int(b[3]))
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (g, kwargs)
        ab = ops.hqq_quantize(w, g, layout="nbits")
        bb = ops.hqq_quantize(w, g, layout="nbits", per_round_launches=True)
        assert torch.equal(ab[0], bb[0]) and torch.equal(ab[2], bb[2])
    # more rounds than the one-pass kernel holds: the per-round route takes over, silently and with the same contract
    c = ops.hqq_quantize(big[:, :520], g, iters=40, early_stop=False)
    d = ops.hqq_quantize(big[:, :520], g, iters=40, early_stop=False, per_round_launches=True)
    assert int(c[3]) == 40 and torch.equal(c[2], d[2]) and torch.equal(c[0], d[0])
