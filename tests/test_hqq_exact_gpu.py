"""HQQ against the oracle, BYTE FOR BYTE at lp_norm = 1 (cases and reasoning: tests/hqq_cases.py; tests/test_hqq_cases.py holds the
CPU half: the oracle equals the restated kernel order on every case here, and every case meets the decision condition).

At lp_norm = 1 the power in the shrink is x^0 = 1 on both sides and every other step is one correctly rounded fp32 operation, so the
scales, the zero points, q [K, N], the MatMulNBits blob and the round count are the oracle's bits -- on the one-pass route and on
the per-round route, at every edge of the 256-column block, for general group sizes (plain loop, tail loop, one and two halvings
of the pairwise tree), for parameters that did not come from RTN, for views and for the 2-byte types.  At any other lp_norm the
zero points are close (tests/test_hqq.py bounds them) and the integers are exact GIVEN the zero points the kernel returned.

A failure prints the (column, k-group) rows that differ with their block (col // 256) and lane.
"""
import numpy as np
import pytest

import hqq_cases as H
import oq_oracle as O

pytestmark = pytest.mark.gpu

ROUTED = [(s, per_round) for s in H.EXACT for per_round in H.routes(s)]


def _route_id(v):
    return H.spec_id(v) if isinstance(v, tuple) else ("per_round" if v else "default")


def _assert_rows(got, want, kgroups, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), f"{what}:\n" + H.describe_rows(got, want, kgroups)


def _assert_integers(q, want, c, what):
    assert q.dtype == np.uint8 and q.shape == want.shape
    if q.tobytes() != want.tobytes():
        k, col = np.nonzero(q != want)
        rows = sorted({(int(n), int(kk) // c.g) for kk, n in zip(k, col)})
        lines = [f"  col {n} k-group {kg} block {n // 256} lane {n % 64}" for n, kg in rows[:12]]
        raise AssertionError(f"{what}: {k.size} integers in {len(rows)} rows differ\n" + "\n".join(lines))


@pytest.mark.parametrize("s, per_round", ROUTED, ids=_route_id)
def test_bit_exact_at_lp_norm_1(s, per_round):
    from onnx_quantize_amd.hip import ops
    c = H.case(s)
    q, sc, z, rounds = c.run(ops, per_round_launches=per_round)
    _assert_rows(sc, c.s, c.kgroups, "scales")
    _assert_rows(z, c.z, c.kgroups, "zero points")
    _assert_integers(q, c.q, c, "q")
    assert rounds == c.rounds
    if c.g % 8 == 0:                                   # the blob needs whole 4-byte words per group
        b, sb, zb, rb = c.run(ops, per_round_launches=per_round, layout="nbits")
        want = c.blob()
        assert b.dtype == np.uint8 and b.shape == want.shape and rb == c.rounds
        _assert_rows(zb, c.z, c.kgroups, "zero points (blob call)")
        if b.tobytes() != want.tobytes():
            n, kg = np.nonzero((b != want).any(axis=2))
            lines = [f"  col {a} k-group {g} block {a // 256} lane {a % 64}" for a, g in list(zip(n.tolist(), kg.tolist()))[:12]]
            raise AssertionError(f"blob: {n.size} rows differ\n" + "\n".join(lines))


@pytest.mark.parametrize("s, lp, per_round", [(s, lp, r) for s, lp in H.ANY_NORM for r in H.routes(s)],
                         ids=lambda v: H.spec_id(v) if isinstance(v, tuple) else str(v))
def test_integers_are_exact_given_the_zero_points(s, lp, per_round):
    """lp_norm 0.5 / 0.7: the hardware's power is not NumPy's, so the zero points are only close (2e-5, test_hqq.py) -- but the finish
    kernel's clip(rint(x / s + z)) is IEEE arithmetic: exact for the z it was given.  The distance to the oracle is printed
    (docs/LAB_NOTES_r33.md records it), not bounded anew."""
    from onnx_quantize_amd.hip import ops
    c = H.case_at(s, lp)
    q, sc, z, rounds = c.run(ops, per_round_launches=per_round)
    _assert_rows(sc, c.s, c.kgroups, "scales")
    dz, moved = float(np.abs(z - c.z).max()), int(np.count_nonzero(q != c.q))
    print(f"\n[hqq lp_norm={lp}] {H.spec_id(s)} per_round={per_round}: max|dz| = {dz:.3e}, {moved} of {q.size} integers differ, "
          f"rounds {rounds} (oracle {c.rounds})")
    _assert_integers(q, H.integers_given(c.w, sc, z, s.group), c, "q given the kernel's zero points")
    assert dz <= 2e-5 and np.abs(q.astype(np.int16) - c.q.astype(np.int16)).max() <= 1
    b = c.run(ops, per_round_launches=per_round, layout="nbits")
    assert b[2].tobytes() == z.tobytes()
    assert b[0].tobytes() == O.matmul_nbits_layout(q, sc, z, c.g, 4, zp_is_float=True)[0].tobytes()


def test_32_rounds_are_the_last_the_one_pass_route_holds():
    """The two routes give the same bits, so only the workspace shows which one ran: the one-pass route keeps the zero points of
    every round there, the per-round route three arrays of them.  32 rounds reach further into the workspace than the forced
    per-round route does; 33 rounds reach exactly as far as that one."""
    import torch
    from onnx_quantize_amd.hip import ops

    def reach(params, **kwargs):
        c = H.case(H.spec(64, 257, kind="abi", params=params))
        ws = torch.full((c.workspace_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
        out = c.run(ops, workspace=ws, **kwargs)
        assert out[3] == c.rounds == c.p["iters"] and out[2].tobytes() == c.z.tobytes()
        return int((ws != 0xA5).nonzero().max()) + 1

    one_pass, per_round, beyond = reach("i32"), reach("i32", per_round_launches=True), reach("i33")
    assert per_round == beyond < one_pass, (one_pass, per_round, beyond)
