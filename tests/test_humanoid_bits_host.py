"""Humanoid host engines: tests/golden/humanoid_fp32_bits.npz (record_humanoid_bits.py) is reproduced word for word.

The device code of humanoid_engine.hpp / humanoid_pair.hpp is held by the assembly comparison (profiles/isa_same.py); the host
instantiations the other humanoid host tests run are held to the oracle within tolerances only, so this fixture is what notices a
refactor that moves host bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import record_humanoid_bits as rec  # noqa: E402


@pytest.fixture(scope="module")
def stored():
    z = np.load(rec.PATH)
    return {k: z[k] for k in z.files}


def test_fixture_reaches_every_solver_path(stored):
    """from the STORED row counts: every dual size, the scratch-row solve_pgs and the no-row path, in each step series; at most 16 states"""
    assert len(stored["states"]) <= 16
    for name in rec.SERIES:
        assert rec.coverage(stored[name + "_nrows"]) == rec.ALL_PATHS, (name, stored[name + "_nrows"])


def test_fixture_bits_are_reproduced(stored):
    """hh_step_rows (default build and -DREX_PGS_CHECK_HOST), hp_step and hp_reset in fp32: every word of qpos, qvel, obs, reward, xout,
    done and nrows equals the recording"""
    want = rec.unpack(stored)
    got = rec.replay(stored["states"], stored["draws"])
    assert set(got) == set(want) - {"states", "draws"}
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (k, len(bad), bad[:8].tolist())
