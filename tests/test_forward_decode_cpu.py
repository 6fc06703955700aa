"""The index arithmetic of the forward composite's phase B1 (dm2_forward_queue.hip, dm2_pairs.h), modelled in numpy:

1. ``(local * ceil(8192 / w)) >> 13 == local // w`` for every local < 256 and w = 1 .. 16, and the reciprocal fits the 16 bits
   the rect word has free (pair_xy, rect_with_inv).
2. The pair -> face decode "start marks + running maximum over the wave + carry between rounds + seed per wave"
   (pair_face_from_marks, pair_face_seed) equals the definition of find_face -- the largest j with off[j] <= k -- for every
   pair of a chunk, with faces that own no pair anywhere in the table."""
import numpy as np
import pytest

PAIRCAP = 768           # DM2_FQ_PAIRCAP
CHUNK = 52              # DM2_FQ_CHUNK


def test_reciprocal_divides_exactly():
    local = np.arange(256, dtype=np.int64)
    for w in range(1, 17):
        inv = (8192 + w - 1) // w
        assert inv < 1 << 16
        assert np.array_equal((local * inv) >> 13, local // w), w
    # (why the old constant had to go: ceil(65536 / 1) needs 17 bits)
    assert (65536 + 1 - 1) // 1 >= 1 << 16


def find_face(off, n, k):
    """dm2_pairs.h: binary search, invariant off[lo] <= k < off[hi]; the largest j < n with off[j] <= k."""
    lo, hi = 0, n
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if off[mid] <= k:
            lo = mid
        else:
            hi = mid
    return lo


def decode_by_marks(cnt):
    """The kernel's phases A and B1 for one chunk: -> (n, tot, face of every pair k < tot)."""
    n = len(cnt)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    # phase A, wave 0: clear, then one mark per face that owns a pair and starts inside the array
    mark = np.zeros(PAIRCAP, dtype=np.uint8)
    for j in range(n):
        if cnt[j] > 0 and off[j] < PAIRCAP:
            assert mark[off[j]] == 0                     # one writer per slot
            mark[off[j]] = j + 1
    tot = int(off[n])
    if tot > PAIRCAP:                                    # cut 1
        n = find_face(off, n, PAIRCAP)
        tot = int(off[n])
    Q = (((tot + 3) >> 2) + 63) & ~63
    assert 4 * Q <= PAIRCAP
    face = np.full(tot, -1, dtype=np.int64)
    for wid in range(4):
        carry = int((off[:n] <= wid * Q).sum())          # the seed: one ballot over the staging lanes
        for r in range(0, Q, 64):
            k = wid * Q + r + np.arange(64)
            mk = np.maximum(np.maximum.accumulate(mark[k].astype(np.int64)), carry)
            carry = int(mk[63])                          # lane 63 of the round
            live = k < tot
            face[k[live]] = mk[live] - 1
    return n, tot, off, face


def check(cnt):
    cnt = np.asarray(cnt, dtype=np.int64)
    assert len(cnt) <= CHUNK and cnt.max(initial=0) <= 256
    n, tot, off, face = decode_by_marks(cnt)
    want = np.array([find_face(off, n, k) for k in range(tot)], dtype=np.int64)
    assert np.array_equal(face, want)
    if tot:
        assert (cnt[face] > 0).all() and (off[face] <= np.arange(tot)).all() and (np.arange(tot) < off[face + 1]).all()
    return tot


@pytest.mark.parametrize("tot", [1, 63, 64, 65, 768])
def test_exact_totals(tot):
    """n = 1 where one face can hold the total, else faces of uneven sizes with gaps, ending exactly at ``tot``."""
    if tot <= 256:
        assert check([tot]) == tot
    rng = np.random.default_rng(tot)
    for _ in range(20):
        cnt = []
        while sum(cnt) < tot:
            cnt.append(int(min(rng.choice([0, 0, 1, 2, 7, 30, 100, 256]), tot - sum(cnt))))
            if len(cnt) == CHUNK - 1:
                break
        if sum(cnt) < tot:
            continue
        cnt = [0] * int(rng.integers(0, 3)) + cnt + [0] * int(rng.integers(0, 3))
        assert check(cnt[:CHUNK]) == tot


def test_runs_of_empty_faces_at_both_ends_and_inside():
    assert check([0, 0, 0, 5, 0, 0, 64, 0, 3, 0, 0, 0]) == 72
    assert check([0] * 51 + [1]) == 1
    assert check([1] + [0] * 51) == 1
    assert check([0, 256, 0, 256, 0, 256, 0]) == 768
    assert check([0] * 10) == 0


def test_cut_at_the_pair_cap():
    """Faces beyond cut 1 keep their marks; no pair in front of the cut may see them."""
    assert check([256, 256, 255, 2, 40]) == 767
    assert check([200, 0, 200, 0, 200, 0, 168, 0, 1]) == 768
    assert check([256, 256, 256, 256]) == 768
    assert check([100] * 9) == 700


def test_random_tables():
    rng = np.random.default_rng(5)
    for it in range(300):
        n = int(rng.integers(1, CHUNK + 1))
        kind = it % 3
        if kind == 0:   cnt = rng.integers(0, 6, n)
        elif kind == 1: cnt = rng.integers(0, 257, n) * (rng.random(n) < 0.3)
        else:           cnt = rng.choice([0, 0, 0, 1, 16, 64, 256], n)
        check(cnt)
