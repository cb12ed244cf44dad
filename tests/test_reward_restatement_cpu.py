"""CPU-only: tests/reward_restatement.py against the rewards `env.step()` of the live reference returned in every recorded `rw_*` run
(oracle/make_golden.py:main_reward), from the recorded states, references and terminated flags alone -- 1e-12 relative, the tolerance
of the other host-derived reference quantities.  The device tests (tests/test_gpu_reward_paths.py) then use the restatement where no
recorded run exists.

Every `rw_*` fixture stores the state of every step (`state_index` is 0 .. K-1, asserted below), so every step is compared."""
import glob
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from reward_restatement import error_terms, full_references, reward  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REWARD_CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "rw_*.npz")))
RTOL = 1e-12


def _load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return d, json.loads(str(d["meta"]))


def test_reward_fixture_inventory():
    """What the recorded runs cover between them: both state lengths, more weighted states than four, general powers beyond four terms."""
    assert len(REWARD_CASES) >= 12
    lengths, n_weighted, general_beyond = set(), set(), False
    for name in REWARD_CASES:
        rw = _load(name)[1]["reward"]
        w, n, refd = np.array(rw["weights"]), np.array(rw["powers"]), np.array(rw["referenced_states"])
        lengths |= {float(x) for x in np.array(rw["state_length"])[w != 0]}
        n_weighted.add(int((w != 0).sum()))
        # the device's term order: referenced states first, then the other weighted states, each in column order
        order = [i for i in range(len(w)) if refd[i]] + [i for i in range(len(w)) if not refd[i] and w[i] != 0]
        general_beyond |= any(n[i] not in (1.0, 2.0) for i in order[4:])
    assert lengths == {1.0, 2.0} and {1, 2, 3, 6, 7} <= n_weighted and general_beyond


@pytest.mark.parametrize("name", REWARD_CASES)
def test_restatement_reproduces_the_recorded_rewards(name):
    d, meta = _load(name)
    rw = meta["reward"]
    K = len(d["rewards"])
    assert np.array_equal(d["state_index"], np.arange(K)) and d["states"].shape == d["references"].shape == (K, len(rw["weights"]))
    refd = np.array(rw["referenced_states"])
    assert not d["references"][:, ~refd].any()  # (the reference's generators return 0 for the states they do not reference)
    term = d["terminated"]
    got = reward(d["states"], d["references"], term, rw["weights"], rw["powers"], rw["state_length"], rw["bias"], rw["violation_reward"])
    want = d["rewards"]
    assert term.sum() > 0 and (got[term] == rw["violation_reward"]).all() and (want[term] == rw["violation_reward"]).all()
    assert np.abs(got - want).max() <= RTOL * np.maximum(1.0, np.abs(want)).max()
    assert np.allclose(got, want, rtol=RTOL, atol=RTOL * abs(rw["bias"]) + 1e-15)
    # the referenced columns alone, scattered by full_references, are the recorded full-width reference
    cols = [i for i, r in enumerate(refd) if r]
    assert np.array_equal(full_references(d["references"][:, cols], cols, len(refd)), d["references"])


def test_restatement_terms_by_hand():
    """Two samples worked by hand: lengths 1 and 2, powers 1, 2, 0.5 and 3, a weight of 0 on a state that holds a NaN."""
    w, n, length = [0.5, 0.25, 0.0, 0.125, 0.125], [1, 2, 1, 0.5, 3], [1, 2, 2, 2, 1]
    s = np.array([[0.5, -1.0, np.nan, 0.5, 1.0], [0.25, 1.0, 7.0, -0.5, 0.5]])
    r = full_references(np.array([[0.25, 0.0], [0.75, 1.0]]), [0, 3], 5)
    assert np.array_equal(r, [[0.25, 0, 0, 0.0, 0], [0.75, 0, 0, 1.0, 0]])
    t = error_terms(s, r, w, n, length)
    want = np.array([[0.5 * 0.25, 0.25 * 0.25, 0.0, 0.125 * 0.5, 0.125], [0.5 * 0.5, 0.25 * 0.25, 0.0, 0.125 * 0.75 ** 0.5, 0.125 * 0.125]])
    assert np.allclose(t, want, rtol=1e-15, atol=0)
    got = reward(s, r, [False, True], w, n, length, 1.0, -3.0)
    assert got[0] == pytest.approx(1.0 - want[0].sum(), rel=1e-15) and got[1] == -3.0
