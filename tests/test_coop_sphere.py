"""The wave-cooperative unit-sphere draw (RT_COOP_SPHERE, pt_core.h / pt_path.h unit_sphere_point) on the CPU: a
64-lane wave emulated over the very functions the device code calls for its assignment arithmetic (which helper
serves which requester at which round offset, how many rounds a requester gets in a trip, the take rule), against
random_in_unit_sphere per lane — the point and the draw count afterwards, bit for bit.  Each requester's first round is
its own; the trips after it are shared."""
import numpy as np
import pytest

import coopcheck_binding as cb


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mask_of(lanes):
    m = 0
    for l in lanes:
        m |= 1 << int(l)
    return m


@pytest.fixture(scope="module")
def pool():
    """400,000 streams (random keys, small draw counts) with the rounds random_in_unit_sphere takes on each"""
    rng = np.random.default_rng(20240611)
    keys = rng.integers(0, 1 << 32, 400_000, dtype=np.uint64).astype(np.uint32)
    k0 = rng.integers(0, 60, 400_000).astype(np.uint32)
    return keys, k0, cb.rounds(keys, k0)


def pick(pool, want, count):
    """`count` streams of the pool whose round count satisfies `want`"""
    keys, k0, r = pool
    at = np.flatnonzero(want(r))[:count]
    assert len(at) == count
    return keys[at], k0[at]


def check_wave(need_lanes, exec_lanes, keys, k0):
    """the emulated wave against the sequential loop on the lanes that need; the others untouched.  Returns the wave."""
    need, ex = mask_of(need_lanes), mask_of(exec_lanes)
    w = cb.wave(need, ex, keys, k0)
    p, k = cb.sequential(keys, k0)
    nl = np.zeros(64, dtype=bool)
    nl[list(need_lanes)] = True
    assert np.array_equal(bits(w["p"][nl]), bits(p[nl]))
    assert np.array_equal(w["k"][nl], k[nl])
    assert np.array_equal(w["k"][~nl], np.asarray(k0, dtype=np.uint32)[~nl]) and not w["p"][~nl].any()
    # every trip consumes at least one round of every requester: no more trips than the slowest lane's own loop
    longest = int(((k[nl] - np.asarray(k0, dtype=np.uint32)[nl]) // 3).max())
    assert w["trips"] + 1 <= longest
    return w


def test_assignment_is_integer_division():
    """q = h mod n, j = h div n and c = H div n + (rho < H mod n) for every h, H <= 64 and n <= 64, also with the
    reciprocal two ulps off either way (the device takes v_rcp_f32's)"""
    assert cb.assign_violations() == 0


def test_random_waves_equal_the_sequential_loop():
    """120,000 random (N, E, keys, k0): every lane's (x, y, z, k) has random_in_unit_sphere's bits, lanes without need
    keep their k, no wave takes more trips than its slowest lane's sequential rounds, and both edges of a trip occur
    (points taken at a requester's last candidate, and at the first of a later trip)."""
    r = cb.random_waves(120_000, 7)
    assert r["lanes"] == 120_000 * 64 and r["bad"] == 0 and r["slow"] == 0
    assert r["last_candidate"] > 1000 and r["next_first"] > 1000


@pytest.mark.parametrize("mutation", [1, 2, 3], ids=["offset+1", "forgets-k+=3c", "takes-offset-c"])
def test_mutations_fail(mutation):
    """an offset shifted by one, a forgotten k += 3 c and a take rule one too wide are all caught"""
    assert cb.random_waves(3000, 7, mutation)["bad"] > 0


def test_every_lane_needs(pool):
    """n = 64 = H: one round per lane and trip"""
    keys, k0 = pick(pool, lambda r: r >= 1, 64)
    check_wave(range(64), range(64), keys, k0)
    keys, k0 = pick(pool, lambda r: r >= 3, 64)
    w = check_wave(range(64), range(64), keys, k0)
    assert w["trips"] >= 2


def test_one_requester_of_a_full_wave(pool):
    """n = 1, H = 64: the requester's next 64 rounds in one trip, the longest streams of the pool included"""
    keys, k0, r = pool
    for at in np.argsort(r)[-4:]:
        kk, k00 = np.full(64, 5, dtype=np.uint32), np.zeros(64, dtype=np.uint32)
        kk[37], k00[37] = keys[at], k0[at]
        w = check_wave([37], range(64), kk, k00)
        assert r[at] >= 12 and w["trips"] == 1


def test_a_single_active_lane(pool):
    """H = 1: the lane's own loop, one round per trip after its first"""
    keys, k0 = pick(pool, lambda r: r >= 5, 64)
    w = check_wave([9], [9], keys, k0)
    assert w["trips"] == cb.rounds(keys[9:10], k0[9:10])[0] - 1


def test_all_but_one_need(pool):
    """n = H - 1: the one helper beyond the requesters serves rank 0 at offset 1, with holes in EXEC"""
    keys, k0 = pick(pool, lambda r: r >= 2, 64)
    lanes = [l for l in range(64) if l % 5 != 3]
    check_wave(lanes[1:], lanes, keys, k0)
    check_wave(lanes[:-1], lanes, keys, k0)


def test_long_rounds_beside_helpers(pool):
    """streams that need at least 12 rounds (about 3e-4 of all keys) among lanes that only help and lanes past the end"""
    keys, k0 = pick(pool, lambda r: r >= 12, 8)
    assert (cb.rounds(keys, k0) >= 12).all()
    kk, k00 = np.arange(64, dtype=np.uint32), np.zeros(64, dtype=np.uint32)
    need = [3, 4, 17, 31, 32, 40, 62, 63]
    kk[need], k00[need] = keys, k0
    check_wave(need, [l for l in range(64) if l not in (0, 5, 33)], kk, k00)
    check_wave(need, range(64), kk, k00)
    check_wave(need, need, kk, k00)


def test_trip_edges(pool):
    """16 requesters of a full wave get c = 4 rounds in the first shared trip: streams accepted at its last candidate
    (offset c - 1) and at the next trip's first (offset c), counted from after the lane's own first round"""
    own = 1
    need = list(range(2, 64, 4))
    for rounds_wanted, flag in ((own + 4, 1), (own + 5, 2)):
        a_keys, a_k0 = pick(pool, lambda r: r == rounds_wanted, 6)
        b_keys, b_k0 = pick(pool, lambda r: (r >= 2) & (r != rounds_wanted), 10)   # none leaves in a plain first round
        kk, k00 = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint32)
        kk[need], k00[need] = np.concatenate([a_keys, b_keys]), np.concatenate([a_k0, b_k0])
        w = check_wave(need, range(64), kk, k00)
        assert (w["flags"][need[:6]] & flag).all()
