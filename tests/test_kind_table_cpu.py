"""gen_inst.py's kind table (KINDS): the one list that the register kernel's
translation units, the SmallVariant rows of inst_table.hip and socp_kernels.hpp's
SmallKind follow.  Read from the generator alone: no library, no GPU.
"""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "socp.jl_amd", "csrc"))
import gen_inst as G  # noqa: E402

CSRC = os.path.dirname(os.path.abspath(G.__file__))


def test_km_suffix_and_position_are_unique():
    n = len(G.KINDS)
    assert len({k.km for k in G.KINDS}) == n
    assert len({k.suffix for k in G.KINDS}) == n
    assert len({k.enum for k in G.KINDS}) == n
    # the position is SmallKind's value: the header lists the same names in the same order
    hdr = open(os.path.join(CSRC, "socp_kernels.hpp")).read()
    body = re.sub(r"//[^\n]*", "", re.search(r"enum SmallKind \{(.*?)\};", hdr, re.S).group(1))
    assert [s.strip() for s in body.split(",")] == ["KIND_" + k.enum for k in G.KINDS] + ["SMALL_KIND_COUNT"]


def test_km_is_the_encoding_of_the_stated_fields():
    """What inst_table.hip's static_asserts hold small_km() to, restated: the bits of socp_small.hpp."""
    for k in G.KINDS:
        assert k.km == k.plugin | k.xi << 1 | k.di << 2 | k.qp << 3 | k.pair << 4 | (G.KM_EXACT if k.exact else 0), k.enum
    assert G.KM_EXACT == 128


def test_slot_and_exact_pairs_are_contiguous_in_pair_order():
    # SLOT_PAIR_* - 1 (socp_small.hpp: SP 1, PS 2, SS 3, PP 4) indexes each run
    names = [k.enum for k in G.KINDS]
    for first in ("SLOT_SP", "EXACT_SP"):
        at = names.index(first)
        assert [k.pair for k in G.KINDS[at:at + 4]] == [1, 2, 3, 4]
        assert names[at:at + 4] == [first[:-2] + p for p in ("SP", "PS", "SS", "PP")]


def test_rows_hold_exactly_the_compiled_kernels():
    for v in G.VARIANTS:
        row = G.row(v)
        assert len(row) == len(G.KINDS)
        assert [k is None or k is G.KINDS[i] for i, k in enumerate(row)] == [True] * len(row)
        assert tuple(k.km for k in row if k) == G.all_kms(v), v
        assert set(G.all_kms(v)) == set(G.kms(v)) | set(G.qp_kkt_kms(v)) | set(G.exact_kms(v))


def test_slot_and_exact_kinds_report_the_plain_solver():
    plain = G.KINDS[0]
    assert plain.km == 0 and plain.entry == "socp_small_kernel"
    for k in G.KINDS:
        if k.pair:
            assert k.entry == plain.entry, k.enum
        else:
            assert k.km == 0 or k.entry != plain.entry, k.enum
    assert len({k.entry for k in G.KINDS if not k.pair}) == sum(1 for k in G.KINDS if not k.pair)


def test_derived_names_keep_their_values():
    assert sum(len(G.kms(v)) for v in G.VARIANTS) == 220 and len(G.VARIANTS) == 36
    assert G.SLOT_KMS == (16, 32, 64)
    assert G.EXACT == [((4, 24, 1), 16)]
    assert G.SUFFIX == {0: "", 1: "_kkt", 2: "_xi", 3: "_xikkt", 4: "_di", 8: "_qp", 9: "_qpkkt",
                        16: "_sp", 32: "_ps", 48: "_ss", 64: "_pp"}
    assert G.kms((4, 24, 1)) == (0, 1, 2, 3, 4, 16, 32, 64, 8) and G.kms((2, 8, 2)) == (0, 1, 4, 8)
    assert G.exact_kms((4, 24, 1)) == (144,) and G.exact_kms((3, 24, 1)) == ()
    assert G.tag((4, 24, 1)) == "q4_p24_m1"


def test_generated_table(tmp_path):
    G.main(str(tmp_path))
    src = (tmp_path / "inst_table.hip").read_text()
    assert src.count("static_assert(KIND_") == len(G.KINDS)
    assert "static_assert(SMALL_KIND_COUNT == %d" % len(G.KINDS) in src
    rows = [ln for ln in src.splitlines() if ln.startswith("  {")]
    assert len(rows) == len(G.VARIANTS)
    for v, ln in zip(G.VARIANTS, rows):
        ents = re.findall(r"\{nullptr, nullptr\}|\{\(const void\*\)&socp_small_kernel<(\d+), (\d+), (\d+), (\d+)>, \"(\w+)<", ln)
        assert len(ents) == len(G.KINDS), v
        assert tuple(int(e[3]) for e in ents if e[3]) == G.all_kms(v)
        for k, e in zip(G.KINDS, ents):
            if e[3]:
                assert (int(e[0]), int(e[1]), int(e[2])) == v and int(e[3]) == k.km and e[4] == k.entry
    files = sorted(p.name for p in tmp_path.iterdir())
    assert len(files) == sum(len(G.all_kms(v)) for v in G.VARIANTS) + 1
    assert "inst_q4_p24_m1_sp_ex.hip" in files and "inst_q2_p12_m1_qpkkt.hip" in files
