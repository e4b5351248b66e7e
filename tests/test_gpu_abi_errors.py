"""The host argument checks of the C-ABI answer what they answered when tests/golden/abi_errors.json was recorded: the same return code and
the same rex_last_error() text, case by case (tests/golden/record_abi_errors.py holds the cases, the handles they run on and why none of them
launches).  The checks run only behind REX_ENTER, so a refactor of the host layer is held to them here: which argument a call with several bad
ones complains about first, every message word for word, and REX_OK without a launch for n == 0."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import record_abi_errors as rec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(rec.PATH))


@pytest.fixture(scope="module")
def replayed():
    """every case run once on fresh handles, shared by the tests below"""
    import __graft_entry__ as g
    g.build()
    c = rec.Ctx()
    try:
        return rec.run(c)
    finally:
        c.close()


def test_the_fixture_holds_the_cases_of_the_recorder(recorded, replayed):
    assert [r["name"] for r in recorded] == [r["name"] for r in replayed]
    assert len(recorded) >= 393 and len(set(r["name"] for r in recorded)) == len(recorded)
    assert set(r["name"].split("/")[0] for r in recorded) >= set(rec.SAMPLE)
    assert all(set(r) == {"name", "rc", "error"} for r in recorded)


def test_every_case_answers_the_recorded_code_and_message(recorded, replayed):
    wrong = [(a["name"], (a["rc"], a["error"]), (b["rc"], b["error"])) for a, b in zip(recorded, replayed) if (a["rc"], a["error"]) != (b["rc"], b["error"])]
    assert not wrong, "%d cases differ (name, recorded, got): %s" % (len(wrong), wrong[:5])


def test_the_recorded_answers_are_refusals_with_the_entry_points_name_or_ok_for_n_0(recorded):
    """the fixture itself: an OK case is one the recorder calls *_ok; every refusal is one of the ABI's codes and, for the sample family, starts
    with the name of the entry point that was called"""
    for r in recorded:
        fn = r["name"].split("/")[0]
        if r["name"].endswith("_ok"):
            assert r["rc"] == 0, r
        else:
            assert r["rc"] in (-1, -3, -4) and r["error"], r
            if fn in rec.SAMPLE:
                assert r["error"].startswith(fn + ": "), r
