"""Shared cases for the inference march away from C = 1, bound = 1, dt_gamma = 0: rays, occupancy, jitter and a toy field
per case, and the reference's eval loop (nerf/renderer.py:526-551) run on the CPU oracle.  tests/test_infer_march_cases_cpu.py
shows that each case reaches what it is meant to reach (several cascade levels, all three step regimes, early termination,
a visible jitter); tests/test_raymarching_gpu.py drives the three inference march kernels through the same cases round by
round.  H = 128 throughout: a Morton index of coordinates below H reaches 2^(3 ceil(log2 H)), which for an H that is no
power of two lies beyond the C H^3-bit bitfield (the reference reads out of range there too; its grid_size is 128)."""
import functools
import types

import numpy as np

from conftest import make_rays, random_bitfield, sphere_bitfield

H = 128
T_THRESH = 1e-2
ALIGN = 128

#        name            N    C  bound  occupancy        dt_gamma  max_steps  seed
CASES = {
    "cone":         (600, 1, 1.0, ("sphere", 0.45), 1 / 128, 256, 40),
    "two_levels":   (300, 2, 2.0, ("sphere", 1.6), 1 / 64, 128, 40),
    "three_levels": (600, 3, 4.0, ("random", None), 1 / 128, 256, 40),
}
NAMES = tuple(CASES)


def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case, built once per process; nobody writes to them."""
    O = _oracle()
    N, C, bound, (kind, radius), dt_gamma, max_steps, seed = CASES[name]
    rng = np.random.default_rng(seed)
    o, d = make_rays(rng, N, bound)
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    nears, fars = O.near_far_from_aabb(o, d, aabb)
    bits = sphere_bitfield(O, C, H, radius) if kind == "sphere" else random_bitfield(rng, C, H)
    noises = rng.random(N).astype(np.float32)

    def field(x):  # deterministic, evaluated on the host for both sides
        s = (6 * np.exp(-np.sum(x * x, 1) / (0.08 * bound * bound))).astype(np.float32)
        c = (0.5 + 0.5 * np.sin(x * 7)).astype(np.float32)
        nrm = (x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-6)).astype(np.float32)
        return s, c, nrm

    for a in (o, d, nears, fars, bits, noises):
        a.setflags(write=False)
    return types.SimpleNamespace(name=name, N=N, C=C, H=H, bound=bound, dt_gamma=dt_gamma, max_steps=max_steps, o=o, d=d,
                                 nears=nears, fars=fars, bits=bits, noises=noises, field=field, T_thresh=T_THRESH)


def dt_limits(c):
    """(dt_min, dt_max) of the march, in float32 as raymarching.cu forms them."""
    s3 = np.float32(1.7320508075688772)
    return np.float32(2) * s3 / np.float32(c.max_steps), np.float32(2) * s3 * np.float32(1 << (c.C - 1)) / np.float32(c.H)


def position_levels(c, xyzs):
    """The cascade level each row's position lies in: the smallest box [-2^l, 2^l]^3 that holds it, clamped to C - 1."""
    return np.clip(np.frexp(np.abs(xyzs).max(1))[1], 0, c.C - 1)


def lookup_levels(c, xyzs, dt):
    """The cascade level the march read each row's occupancy bit from: max(level of the position, level of the step),
    clamped.  The step's level is the exponent of dt H / 2, so a dt_min of 2 sqrt(3) / max_steps >= 2 / H (max_steps <=
    sqrt(3) H) keeps every lookup out of level 0."""
    ld = np.frexp(dt * np.float32(0.5 * c.H))[1]
    return np.clip(np.maximum(position_levels(c, xyzs), ld), 0, c.C - 1)


@functools.lru_cache(maxsize=None)
def reference_loop(name, perturb, jitter_every_round=False):
    """The loop of nerf/renderer.py:526-551 on the CPU oracle: march_rays (noises in round 0 only, noises[:n_alive]
    indexed by alive slot; jitter_every_round = the mistake of handing them to every round), the toy field,
    composite_rays, the boolean-mask compaction.  Returns (rounds, final): per round the loop state before it (n_alive,
    n_step, step, alive, t), the march's rows and the state after the composite (alive_after with its -1 marks, t_after);
    final = the accumulators and the state the loop ends in."""
    O = _oracle()
    c = case(name)
    N = c.N
    ws, dep = np.zeros(N, np.float32), np.zeros(N, np.float32)
    img, nrm = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    alive, t = np.arange(N, dtype=np.int32), c.nears.copy()
    step, rounds = 0, []
    while step < c.max_steps:
        n_alive = alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        noises = c.noises[:n_alive] if perturb and (step == 0 or jitter_every_round) else None
        xyzs, dirs, deltas = O.march_rays(n_alive, n_step, alive, t, c.o, c.d, c.bound, c.bits, c.C, H, c.nears, c.fars,
                                          align=ALIGN, noises=noises, dt_gamma=c.dt_gamma, max_steps=c.max_steps)
        rec = types.SimpleNamespace(n_alive=n_alive, n_step=n_step, step=step, alive=alive.copy(), t=t.copy(), xyzs=xyzs,
                                    dirs=dirs, deltas=deltas)
        s, col, nm = c.field(xyzs)
        O.composite_rays(n_alive, n_step, alive, t, s, col, nm, deltas, ws, dep, img, nrm, c.T_thresh)
        rec.alive_after, rec.t_after = alive.copy(), t.copy()
        rounds.append(rec)
        alive = alive[alive >= 0]
        step += n_step
    final = types.SimpleNamespace(weights_sum=ws, depth=dep, image=img, normal=nrm, alive=alive, t=t, step=step)
    for rec in rounds:
        for a in vars(rec).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    for a in vars(final).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(rounds), final


def emitted(rounds):
    """All rows the loop emitted (delta != 0), concatenated over the rounds: (xyzs, dt)."""
    xs = [r.xyzs[:r.n_alive * r.n_step][r.deltas[:r.n_alive * r.n_step, 0] != 0] for r in rounds]
    ds = [r.deltas[:r.n_alive * r.n_step, 0][r.deltas[:r.n_alive * r.n_step, 0] != 0] for r in rounds]
    return np.concatenate(xs), np.concatenate(ds)
