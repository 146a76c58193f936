"""The table forms of the fused half RTN kernels (csrc/rtn_half.hip: rtn_half_wave_many, rtn_half_column_many) against their
single-matrix twins, from the compiler's own resource report (hipcc cross-compiles without a GPU).

Both forms run ONE __device__ body; the table form adds four scalar loads and the [K, N/2] epilogue.  The 16-row build with
16-byte loads sits right at the boundary of three waves per SIMD (docs/LAB_NOTES_r07.md), so neither addition may cost a wave or
scratch traffic there.  The kernels are compared with each other: no figure of a particular compiler is written down here."""
from kernel_report import needs_hipcc, report


@needs_hipcc
def test_table_kernels_keep_the_occupancy_of_their_single_matrix_twins():
    seen = {name: (k.scratch, k.occupancy) for name, k in report("rtn_half.hip").kernels.items()}
    pairs = []
    for elem in ("NS_7ElemF16E", "NS_8ElemBF16E"):
        for rows in (16, 32):
            for vec in (1, 0):
                build = f"I{elem}Li{rows}ELb{vec}EEEv"
                pairs.append((rows == 16 and vec == 1, f"_ZN2oq13rtn_half_wave{build}NS_8HalfArgsE",
                              f"_ZN2oq18rtn_half_wave_many{build}NS_8HalfArgsEPKNS_8HalfPtrsE"))
        pairs.append((False, f"_ZN2oq15rtn_half_columnI{elem}EEvNS_8HalfArgsE", f"_ZN2oq20rtn_half_column_manyI{elem}EEvNS_8HalfArgsEPKNS_8HalfPtrsE"))
    assert len(pairs) == 10
    for hot, single, many in pairs:
        assert single in seen and many in seen, (single, many, sorted(seen))
        (s_scratch, s_occ), (m_scratch, m_occ) = seen[single], seen[many]
        if hot:       # the 16-row build with 16-byte loads: the occupancy of the twin and no more scratch than it
            assert m_occ == s_occ and m_scratch <= s_scratch, (many, seen[many], seen[single])
        else:         # every other build: no scratch where the twin has none
            assert m_scratch == 0 or s_scratch > 0, (many, seen[many], seen[single])
