"""Prioritised sampling over the transition ring (include/procgen2_vec.h pgv_priorities_enable), the GPU half: the HIP
sampler against a numpy model that follows the header's point 5 literally — uint64 weights, cumsum, targets in Python
integers, searchsorted, np.float32 for prob — bit for bit.  The ring is driven to a chosen head by real synthetic steps of
maze; the flag bytes are then overwritten through the zero-copy view with patterns play would take long to reach, and the
priorities given through transition_priorities, whose fixed point is held to the header's point 2 on the way.

Shapes: (N 3, T 4, head 3) one partial chunk, ring not yet full — once with priorities so small that S < 4096 and a
stratified call of 4096 has parts of width zero; (131, 40, 57) two chunks, rows wrapped, a chunk straddling slots, N no
multiple of 16; (4099, 3, 8) four chunks; (65537, 16, 19) 257 chunks, the smallest ring whose chunk sums take the scan a
second pass, and two rounds of the chunk search.  The last test is one law end to end on bossfight, whose episodes end often under
random play and whose plain steps record VOID rows.
"""
import numpy as np
import pytest
import torch

from history_aug_util import word
from procgen2_amd import lib as pglib
from procgen2_amd.vec_env import ProcgenVecEnv
from transitions_util import RECORDED, VOID, entries

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4, 3, "tiny"), (3, 4, 3, "mixed"), (131, 40, 57, "mixed"), (4099, 3, 8, "mixed"), (65537, 16, 19, "mixed")]
COUNTS = (1, 7, 4096)
TOP = 2147483647


def fix(values):
    """Point 2 in np.float32."""
    t = np.asarray(values, np.float32) * np.float32(65536.0)
    small, big = ~(t >= np.float32(1.0)), t >= np.float32(2147483648.0)
    middle = np.rint(np.where(small | big, np.float32(1.0), t)).astype(np.int64)  # (exact: below 2^31)
    return np.where(big, TOP, np.where(small, 1, middle)).astype(np.uint32)


def slot_rows(head, T):
    """The row living in every slot (-1: none yet), and whether it is held with its successor."""
    row = np.full(T, -1, np.int64)
    for q in range(max(0, head - T), head):
        row[q % T] = q
    return row, (row >= 0) & (row >= head - T) & (row + 1 < head)


def sample_model(flags, priority, head, count, seed, stratified):
    """Point 5: (pushes, envs, priority, prob, S, M)."""
    T, N = flags.shape
    row, held = slot_rows(head, T)
    eligible = held[:, None] & ((flags & RECORDED) != 0) & ((flags & VOID) == 0)
    w = np.where(eligible, priority, 0).astype(np.uint64).reshape(-1)
    cum = np.cumsum(w, dtype=np.uint64)
    S, M = int(cum[-1]), int(eligible.sum())
    if S == 0:
        return np.full(count, -1, np.int64), np.full(count, -1, np.int32), np.zeros(count, np.uint32), np.zeros(count, np.float32), S, M
    words = [int(x) for x in word(seed, np.arange(count), 0)]
    lo = [k * S // count for k in range(count + 1)] if stratified else [0] * count + [S]
    targets = []
    for k in range(count):
        width = (lo[k + 1] - lo[k]) if stratified else S
        targets.append(lo[k] + words[k] * (width >> 32) + ((words[k] * (width & 0xFFFFFFFF)) >> 32))
    j = np.searchsorted(cum, np.array(targets, np.uint64), side="right")
    prob = w[j].astype(np.float32) / np.array([S], np.uint64).astype(np.float32)
    return row[j // N], (j % N).astype(np.int32), w[j].astype(np.uint32), prob.astype(np.float32), S, M


def ring_at(game, N, T, head, **more):
    """An engine whose ring stands at `head` pushes: the reset's frame, then head - 1 synthetic steps."""
    v = ProcgenVecEnv(game, N, seed_base=1, history=dict(capacity=T, gray=True), transitions=True, priorities=True, **more)
    v.reset()
    for _ in range(head - 1):
        v.step_synthetic(7)
    assert v.history.head == head
    return v


def check_sample(v, flags, priority, head, count, seed, stratified):
    got = v.transition_sample(count, seed, stratified=stratified)
    pushes, envs, pr, prob, S, M = sample_model(flags, priority, head, count, seed, stratified)
    what = (count, seed, stratified)
    assert (int(got.total), int(got.eligible)) == (S, M), what
    assert np.array_equal(got.pushes.cpu().numpy(), pushes), what
    assert np.array_equal(got.envs.cpu().numpy(), envs), what
    assert np.array_equal(got.priority.cpu().numpy().view(np.uint32), pr), what
    assert np.array_equal(got.prob.cpu().numpy().view(np.uint32), prob.view(np.uint32)), what
    return got


@pytest.mark.parametrize("stratified", [True, False])
@pytest.mark.parametrize("N,T,head,kind", SHAPES)
def test_sample_is_the_model_bit_for_bit(N, T, head, kind, stratified):
    rng = np.random.default_rng(N + head)
    v = ring_at("maze", N, T, head)
    flags = rng.choice(np.array([0, 1, 1, 1, 3, 5, 9, 11, 17], np.uint8), size=(T, N))
    v.transitions.flags.copy_(torch.from_numpy(flags))
    # a priority for every held row, and for entries that name none: those are skipped
    p, i = entries(head, T, N)
    named = (i >= 0) & (i < N) & (p >= 0) & (p >= head - T) & (p + 1 < head)
    special = np.array([0.0, np.nan, 1e-9, 1e-4], np.float32)
    values = np.where(rng.random(p.size) < (1.0 if kind == "tiny" else 0.1), rng.choice(special, p.size), rng.uniform(0, 4, p.size)).astype(np.float32)
    if kind == "mixed":  # the top of the fixed point, on two rows only: they take most of S, not all of it
        values[np.flatnonzero(named)[[0, 1, -1]]] = 3e4, 0.0, np.inf
    v.transition_priorities(p, i, values)
    priority = np.full((T, N), pglib.PRIORITY_ONE, np.uint32)  # what the enable and every opened row left
    priority[p[named] % T, i[named]] = fix(values[named])
    assert np.array_equal(v.transitions.priority.cpu().numpy().view(np.uint32), priority)
    assert int(v.transitions.priority_max.item()) == max(pglib.PRIORITY_ONE, int(fix(values[named]).max()))
    assert kind == "tiny" or {1, TOP} <= set(priority.reshape(-1).tolist())  # both ends of the fixed point
    for count in COUNTS:
        got = check_sample(v, flags, priority, head, count, 5 + count, stratified)
        assert int(got.eligible) >= 2 and (kind != "tiny" or int(got.total) < 4096)
    again = v.transition_sample(4096, 5 + 4096, stratified=stratified)  # the same seed, the same bytes; the engine unchanged
    assert all(torch.equal(a, b) for a, b in zip(again, got)) and v.history.head == head
    v.transitions.flags.zero_()  # nothing eligible: S = 0
    got = check_sample(v, np.zeros_like(flags), priority, head, 7, 1, stratified)
    assert int(got.total) == 0 and int(got.eligible) == 0 and bool((got.pushes == -1).all()) and bool((got.envs == -1).all())
    v.close()


def test_samples_are_valid_transitions_and_new_rows_open_at_the_maximum():
    N, T = 131, 40
    v = ring_at("bossfight", N, T, 41)
    assert bool(((v.transitions.flags & VOID) != 0).any()), "the run has resets' own steps to avoid"
    s = v.transition_sample(512, 3)
    assert int(s.eligible) > 0 and bool((s.priority == pglib.PRIORITY_ONE).all())
    t = v.transition_gather(s.pushes, s.envs, n=1, frames=False)
    assert bool(((t.status & 1) == 1).all())
    assert not bool(((v.transitions.flags[s.pushes % T, s.envs.long()] & VOID) != 0).any())
    v.transition_priorities(s.pushes[:8], s.envs[:8], torch.full((8,), 3.0))
    for _ in range(2):
        v.step_synthetic(7)
    head = v.history.head
    for q in (head - 2, head - 3):  # the rows the two steps recorded
        assert bool((v.transitions.priority[q % T] == 3 * pglib.PRIORITY_ONE).all())
    assert int(v.transitions.priority_max.item()) == 3 * pglib.PRIORITY_ONE
    v.close()
