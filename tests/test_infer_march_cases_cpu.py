"""CPU only: the cases of tests/infer_march_cases.py reach what they are meant to reach, on the oracle's own loop.  A case
whose rows all sat in cascade 0, whose steps were all dt_min, whose rays never terminated early or whose jitter moved
nothing visible would let the GPU tests built on it pass over a wrong dt_max, a wrong cascade lookup or a misplaced
jitter; every bound below is far from what the cases measure (printed with -s)."""
import numpy as np
import pytest

import infer_march_cases as IM


def _dt_regimes(c, dt):
    dt_min, dt_max = IM.dt_limits(c)
    assert dt.min() >= dt_min and dt.max() <= dt_max
    return int((dt == dt_min).sum()), int((dt == dt_max).sum()), int(((dt > dt_min) & (dt < dt_max)).sum())


def _levels(name):
    """(case, rows, dt, rows per level by position, rows per level the march looked up)."""
    c = IM.case(name)
    rounds, _ = IM.reference_loop(name, False)
    x, dt = IM.emitted(rounds)
    return (c, x, dt, np.bincount(IM.position_levels(c, x), minlength=c.C),
            np.bincount(IM.lookup_levels(c, x, dt), minlength=c.C))


def test_two_levels_splits_rows_and_steps():
    """Rows inside and outside the unit box, and dt in all three regimes.  (The occupancy LOOKUP of this case is always
    level 1: max_steps = 128 makes dt_min H / 2 = sqrt(3), whose level is 1 - so the rows inside the unit box are the
    ones whose level comes from the step and not from the position.)"""
    c, x, dt, per_level, looked_up = _levels("two_levels")
    n = dt.shape[0]
    at_min, at_max, between = _dt_regimes(c, dt)
    print(f"two_levels: rows per level {per_level.tolist()} of {n} (looked up in {looked_up.tolist()}); dt at dt_min / "
          f"dt_max / between {at_min} / {at_max} / {between}")
    assert n > 5000 and at_min + at_max + between == n
    assert (per_level >= 0.2 * n).all()
    assert min(at_min, at_max, between) >= 0.1 * n
    assert looked_up.tolist() == [0, n]


def test_three_levels_reaches_every_level():
    c, x, dt, per_level, looked_up = _levels("three_levels")
    n = dt.shape[0]
    print(f"three_levels: rows per level {per_level.tolist()} of {n} (looked up in {looked_up.tolist()})")
    assert n > 5000 and (per_level >= 0.03 * n).all()
    assert (looked_up > 0).all()                                # every cascade's bits are read


def test_cone_steps_below_dt_max():
    c, x, dt, per_level, _ = _levels("cone")
    n = dt.shape[0]
    at_min, at_max, between = _dt_regimes(c, dt)
    print(f"cone: dt at dt_min / dt_max / between {at_min} / {at_max} / {between} of {n}")
    assert at_max == 0 and at_min >= 0.3 * n and between >= 0.3 * n


@pytest.mark.parametrize("name", IM.NAMES)
@pytest.mark.parametrize("perturb", [False, True])
def test_loops_terminate(name, perturb):
    c = IM.case(name)
    rounds, final = IM.reference_loop(name, perturb)
    print(f"{name} perturb={perturb}: {len(rounds)} rounds, {final.step} steps, weights_sum max "
          f"{final.weights_sum.max():.4f}")
    assert final.weights_sum.max() > 0.94                       # some rays end on T < T_thresh
    assert final.alive.shape[0] == 0 and len(rounds) <= c.max_steps
    assert rounds[0].n_alive == c.N and rounds[0].n_step == 1 and len(rounds) >= 3
    assert any(r.n_step > 1 for r in rounds)                    # rows laid out at n * n_step with n_step > 1


@pytest.mark.parametrize("name", IM.NAMES)
def test_jitter_is_visible(name):
    plain, jit = IM.reference_loop(name, False), IM.reference_loop(name, True)
    every = IM.reference_loop(name, True, jitter_every_round=True)
    diff = float(np.abs(jit[1].image - plain[1].image).max())
    print(f"{name}: perturbed image differs from the unperturbed by {diff:.3g}")
    assert diff > 1e-3                                          # >= 10 x the 1e-4 the GPU tests compare at
    # round 0 is the same march; from round 1 on a jitter in every round shows
    for k in ("xyzs", "dirs", "deltas"):
        assert np.array_equal(getattr(jit[0][0], k), getattr(every[0][0], k))
    a, b = jit[0][1], every[0][1]
    assert np.array_equal(a.alive, b.alive) and np.array_equal(a.t, b.t)
    assert not np.array_equal(a.xyzs, b.xyzs)
    # in round 0 of the loop slot == ray id: a jitter looked up by ray id shows only on an alive list in another order,
    # which the GPU tests hand the kernels in a round of its own
    assert np.array_equal(jit[0][0].alive, np.arange(jit[0][0].n_alive))
