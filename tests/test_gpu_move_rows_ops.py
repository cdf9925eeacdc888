"""The launches that move rows and step states between the arithmetic kernels, each alone (fl_op_move_rows) against the index formulas
of tests/step_ref.py.  Every destination comes back whole between two guard bands: the payload must equal the reference bit for bit --
a word nobody wrote keeps the all-ones fill and fails that -- and the bands must still be the fill.  Every case asserts through the
launch counts that it reached the launcher it names.  What backs each case's data: test_step_ref.py."""
import numpy as np
import pytest

import step_ref as S

pytestmark = pytest.mark.gpu
FILL = S.FILL
G = 64


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1 and fastllm_amd.MOVE_ROWS_GUARD == G
    return fastllm_amd


def payload(whole):
    """the words between the guard bands, after checking the bands (last axis)"""
    assert (whole[..., :G] == FILL).all() and (whole[..., -G:] == FILL).all(), "a guard band was written"
    return whole[..., G:-G]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_TABLES = {}


def table(dtype, h):
    """[300, h]: every element its own value -- bf16 bit patterns of finite numbers, or float32 that no bf16 holds"""
    if (dtype, h) not in _TABLES:
        rng = np.random.default_rng(h)
        if dtype == "bf16":
            t = rng.integers(0x3000, 0x4800, size=(300, h)).astype(np.uint16) | (rng.integers(0, 2, size=(300, h)).astype(np.uint16) << 15)
        else:
            t = (rng.normal(size=(300, h)) + np.float32(1e-4)).astype(np.float32)
        _TABLES[(dtype, h)] = t
    return _TABLES[(dtype, h)]


IDS = {1: [299], 5: [0, 299, 7, 7, 150], 8: [299, 0, 0, 12, 299, 5, 77, 298], 33: [0, 299] + [(37 * i) % 300 for i in range(31)]}


@pytest.mark.parametrize("dtype", ("bf16", "f32"))
@pytest.mark.parametrize("h", (8, 64, 2056, 4096))         # 2056: the 256 lanes wrap once and leave a one-chunk tail
def test_embed(fa, dtype, h):
    tab = table(dtype, h)
    for T in (1, 5):
        whole, launches = fa.op_embed_rows(tab, IDS[T])
        assert launches == (1, 0)
        assert (payload(whole) == u32(S.embed(tab, IDS[T])).reshape(-1)).all(), T
    whole, launches = fa.op_embed_rows(tab, [150], use_state=True)          # the decode step's form: the id from the step state
    assert launches == (1, 0) and (payload(whole) == u32(S.embed(tab, [150])).reshape(-1)).all()


@pytest.mark.parametrize("dtype", ("bf16", "f32"))
@pytest.mark.parametrize("h", (8, 64, 2056, 4096))
def test_embed_batch(fa, dtype, h):
    tab = table(dtype, h)
    for B in (1, 8, 33):
        whole, launches = fa.op_embed_rows(tab, IDS[B], batch=True)
        assert launches == (1, 0)
        assert (payload(whole) == u32(S.embed(tab, IDS[B])).reshape(-1)).all(), B


@pytest.mark.parametrize("tp", (2, 4, 8))
@pytest.mark.parametrize("B", (1, 3, 8))
def test_unshard_logits(fa, tp, B):
    for Vs in (4, 1000, 4004):                             # n / 4 = tp * B * Vs / 4: below 256 at Vs = 4, no multiple of 256 at 1000 x 3
        src = np.arange(tp * B * Vs, dtype=np.float32).reshape(tp, B, Vs)
        whole, launches = fa.op_unshard_logits(src)
        assert launches == (1, 0)
        assert (payload(whole) == u32(S.unshard(src)).reshape(-1)).all(), Vs
    assert (2 * 1 * 4) // 4 < 256 and (tp * 3 * 1000 // 4) % 256 != 0


@pytest.mark.parametrize("counts", ([1], [3, 1, 7], [2, 1, 5, 1, 1, 9, 4, 1, 3]))
@pytest.mark.parametrize("h", (4, 1028, 4096))
def test_gather_last_rows(fa, counts, h):
    T, n = sum(counts), len(counts)
    for n_slab in (1, 3):
        src_slab, dst_slab = T * h + 12, n * h + 20        # both looser than the rows they hold
        rng = np.random.default_rng(T + h + n_slab)
        src = rng.normal(size=(n_slab, src_slab)).astype(np.float32)
        whole, launches = fa.op_gather_last_rows(src, counts, h, dst_slab)
        assert launches == (1, 0)
        want = S.gather_last_rows(u32(src), counts, h, dst_slab, FILL)      # the 20 floats behind each slab's rows keep the fill
        assert (payload(whole) == want.reshape(-1)).all(), n_slab


@pytest.mark.parametrize("nshards", (1, 2, 4, 8))
def test_reduce_shards(fa, nshards):
    for n in (1, 255, 256, 257, 100003):
        src = S.shard_data(nshards, n)
        whole, launches = fa.op_reduce_shards(src)
        assert launches == (1, 0) and whole.shape == (nshards, n + 2 * G)
        want = u32(S.reduce_shards(src))
        for k in range(nshards):
            assert (payload(whole[k]) == want).all(), (n, k)
        if nshards >= 3:                                   # ... which the sum from the other end does not meet (test_step_ref.py)
            assert (payload(whole[0]) != u32(S.reduce_shards(src, reverse=True))).any()


def member_samplers(fa, n):
    """ArgMax, plain, top-p and top-k members in turn, each with a seed and a stream position of its own"""
    out = []
    for s in range(n):
        kind = s % 4
        out.append(None if kind == 0 else fa.make_sampler(0.5 + 0.01 * s, 1000 + s, 3 * s, 0.9 if kind == 2 else None, 11 if kind == 3 else None))
    return out


@pytest.mark.parametrize("n_seq,n_tickets", ((1, 0), (5, 1), (64, 64), (65, 65), (130, 200), (5, 200), (130, 0)))
def test_packed_set_states_and_collect(fa, n_seq, n_tickets):
    s = np.arange(n_seq, dtype=np.uint32)
    tokens, pos, lens = 7 + 3 * s, 100 + 5 * s, 20 + s
    plant_t, plant_e = 50000 + 11 * s, np.where(s % 3 == 0, 0, 0xE000 + s).astype(np.uint32)
    res = fa.op_packed_states(tokens, pos, lens, n_tickets, plant_t, plant_e, samplers=member_samplers(fa, n_seq))
    assert res.launches == (1, 1)
    for i in range(n_seq):
        assert S.state_tuple(res.states[i]) == S.state_tuple(S.packed_state(int(tokens[i]), int(pos[i]), int(lens[i]))), i
    # the token selection state: a byte copy of the member's init, and the members' inits differ
    assert (res.ss == res.ss_init).all() and (res.ss_init != FILL).any(axis=1).all()
    if n_seq > 5:
        assert (res.ss_init[1] != res.ss_init[5]).any() and res.ss_init[0, 0] == 0 and res.ss_init[1, 0] != 0
    # exactly n_tickets words zeroed per member
    assert (res.tickets[:, :n_tickets] == 0).all() and (res.tickets[:, n_tickets:] == FILL).all()
    assert (payload(res.collect) == S.collect(plant_t, plant_e)).all()


def test_packed_set_states_without_tickets(fa):
    """n_tickets == 0 and no ticket memory at all: the kernel gets a null pointer and must not touch it"""
    res = fa.op_packed_states([4, 5], [1, 2], [8, 9], 0, [6, 7], [0, 3], tickets=False)
    assert res.launches == (1, 1) and res.tickets is None
    assert [S.state_tuple(r) for r in res.states] == [S.state_tuple(S.packed_state(4, 1, 8)), S.state_tuple(S.packed_state(5, 2, 9))]
    assert (res.ss == 0).all() and (payload(res.collect) == [6, 0, 7, 3]).all()
