"""k_bed_size / k_bed_fill on the device through the test hook uz_bed_rows_lists: the hand-built panel (tests/bedcases.py) byte for byte
against summarize.bed_lines, and the refusals of uz_bed_rows / uz_bed_rows_lists."""
import numpy as np
import pytest

import bedcases
from unfazed_amd import abi
from unfazed_amd.engine import UnfazedHipError

pytestmark = pytest.mark.gpu


def _run(engine, case, p=None, names=True):
    p = p or bedcases.pack(case)
    return engine.bed_rows_lists(p["rows"], p["str_off"], p["str_bytes"], case["verbose"], case["include_ambiguous"], p["status"], p["list_off"], p["list_val"],
                                 p["name_off"] if names else None, p["name_bytes"] if names else None, case["ratio"])


@pytest.fixture(scope="module")
def expected():
    return {c["name"]: bedcases.expected_rows(c) for c in bedcases.CASES}  # (computed once, never changed)


def test_the_panel_byte_for_byte(engine, expected):
    bad = []
    for c in bedcases.CASES:
        text, off = _run(engine, c)
        want = expected[c["name"]]
        assert off.size == len(want) + 1 and off[0] == 0
        got = [text[int(off[k]): int(off[k + 1])] for k in range(len(want))]
        if got != want or int(off[-1]) != len(text):
            bad.append(c["name"])
    assert not bad, bad


def test_a_fuzz_of_rows_byte_for_byte(engine):
    for c in bedcases.fuzz_cases(77, 600, rows_per_case=200):
        text, off = _run(engine, c)
        want = bedcases.expected_rows(c)
        assert [text[int(off[k]): int(off[k + 1])] for k in range(len(want))] == want, c["name"]


def _case(lists, verbose=True, n_names=4):
    return dict(name="x", ratio=10, include_ambiguous=False, verbose=verbose, names=["n%d" % k for k in range(n_names)], dnms=[dict(status=0, lists=lists)],
                rows=[bedcases._row(0)])


def _code(exc):
    return int(str(exc.value).split("(")[1].split(")")[0])


def test_a_name_id_out_of_range_is_refused(engine):
    for ids in ([0, 1, 4], [1000000], [-1]):  # (the store holds four names)
        with pytest.raises(UnfazedHipError) as e:
            _run(engine, _case((ids, [], [5], [])))
        assert _code(e) == -4


def test_a_site_list_not_ascending_is_refused(engine):
    for sites in ([10, 9], [5, 5], [-1, 3]):
        with pytest.raises(UnfazedHipError) as e:
            _run(engine, _case(([0], [], sites, [])))
        assert _code(e) == -4


def test_verbose_without_names_is_refused_and_plain_rows_need_none(engine):
    c = _case(([0, 1], [], [5], []))
    with pytest.raises(UnfazedHipError) as e:
        _run(engine, c, names=False)
    assert _code(e) == -4
    plain = dict(c, verbose=False)
    text, off = _run(engine, plain, names=False)
    assert [text] == bedcases.expected_rows(plain) and int(off[1]) == len(text)


def test_a_dnm_index_or_string_id_out_of_range_is_refused(engine):
    c = _case(([0], [], [5], []))
    p = bedcases.pack(c)
    for field, value in (("dnm", 1), ("kid", 99)):
        q = dict(p, rows=p["rows"].copy())
        q["rows"][field][0] = value
        with pytest.raises(UnfazedHipError) as e:
            _run(engine, c, q)
        assert _code(e) == -1


def test_no_finished_batch_is_refused(hip_lib):
    from unfazed_amd.engine import HipEngine
    e2 = HipEngine(0)  # a context that has run no batch
    try:
        st = abi.StringTable()
        rows = np.zeros(1, abi.BED_ROW)
        rows[0] = (0, 1, 2, st.id("chr1"), st.id("POINT"), st.id("k"), st.id("d"), st.id("m"), -1, 0)
        with pytest.raises(UnfazedHipError) as e:
            e2.bed_rows(rows, *st.arrays(), False, False)
        assert _code(e) == -4
    finally:
        e2.close()
