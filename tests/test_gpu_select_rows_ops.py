"""Token selection's launches alone (fl_op_select_rows) against tests/step_ref.py: every field of every member's step state, the
out_tokens buffer WHOLE (a slot nobody wrote keeps the fill pattern), the sampler's kept count and the log-prob records in their state
forms.  All comparisons are equalities.  ArgMax tokens come from the reference; sampled tokens from op_sample and record contents from
op_logprobs, the entry points with tests of their own against the oracle.  Every case asserts through the launch counts that it
reached the launcher it names.  What backs each case's data: test_step_ref.py."""
import numpy as np
import pytest

import step_ref as S
from logit_rules_ref import argmax_last

pytestmark = pytest.mark.gpu
FILL = S.FILL
VS = (151, 1003, 32000, 40000)          # 151, 1003: the scalar walk; 32000: one trip of the 16-byte walk; 40000: two


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def pack(fa, dicts):
    st = np.zeros(len(dicts), fa.STEP_STATE)
    for i, d in enumerate(dicts):
        for f in S.STATE_FIELDS:
            st[f][i] = d[f]
    return st


def start_states(rows, seed=0):
    """one start state per logits row: steps 0 and 5, pos != len, and in turn no EOS / the id that wins / an id that does not / done
    preset beside an EOS that does not match; error and call0 hold values nobody may touch"""
    out = []
    for r, row in enumerate(rows):
        win = argmax_last(row)
        kind = (r + seed) % 4
        eos = (-1, win, (win + 1) % len(row), (win + 2) % len(row))[kind]
        out.append(S.state(token=1000 + r, pos=40 + 3 * r, len=17 + r, step=(0, 5)[(r + seed) % 2], eos=eos, done=1 if kind == 3 else 0,
                           error=0x1234 + r, call0=77 + r))
    return out


def check_member(res, b, st0, tokens, advance, cap):
    st, out, _ = S.select_run(st0, tokens, advance, cap)
    assert S.state_tuple(res.states[b]) == S.state_tuple(st), (b, res.states[b], st)
    assert (res.out_tokens[b] == out).all(), (b, res.out_tokens[b], out)
    return st


@pytest.mark.parametrize("V", VS)
def test_select_single_state_machine(fa, V):
    rows = S.tie_rows(V)
    wins = [argmax_last(r) for r in rows]
    cap = 12
    for advance in (0, 1):
        for n_steps in (1, 4):
            sts = start_states(rows, seed=advance)
            res = fa.op_select_rows(rows, pack(fa, sts), form=0, advance=advance, n_steps=n_steps, out_cap=cap)
            assert res.launches == (len(rows) * n_steps, 0, 0)
            for b, st0 in enumerate(sts):
                st = check_member(res, b, st0, [wins[b]] * n_steps, advance, cap)
                written = np.flatnonzero(res.out_tokens[b] != FILL)
                assert list(written) == ([st0["step"]] if advance == 0 else list(range(st0["step"], st0["step"] + n_steps)))
                assert (st["error"], st["call0"]) == (st0["error"], st0["call0"])
                assert st["done"] == (1 if st0["done"] or st0["eos"] == wins[b] else 0)
                if st0["done"]:                                         # selection goes on after `done`: the host stops the loop
                    assert int(res.states["token"][b]) == wins[b] != st0["token"] and int(res.out_tokens[b, st0["step"]]) == wins[b]
            assert (res.kept == V).all()


def test_select_single_agrees_with_verify_select_on_nan(fa):
    """NaN ordering is pinned between the kernels, not against the oracle: one ArgMax body serves both"""
    rng = np.random.default_rng(5)
    rows = rng.normal(size=(3, 1003)).astype(np.float32)
    rows[0, [0, 500, 1002]] = np.nan
    rows[1, 7] = np.nan
    rows[1, 8] = np.inf
    rows[2, :] = np.nan
    rows[2, 600] = 1.0
    res = fa.op_select_rows(rows, pack(fa, [S.state()] * 3), form=0, n_steps=1)
    for b in range(3):
        assert int(res.states["token"][b]) == int(fa.op_verify_select(rows[b:b + 1], [])[0][0]), b


@pytest.mark.parametrize("count", (1, 2, 64, 65, 1023))
def test_select_candidates_tie_rule_and_count(fa, count):
    V = 4096
    lg = np.zeros((1, V), np.float32)
    lg[0, 11] = 50.0                                                    # the vocabulary's own ArgMax: not a candidate, so reading the row shows
    for descending in (False, True):
        idx = np.arange(count, dtype=np.int32) * 4 + 1
        if descending:
            idx = idx[::-1].copy()                                      # the larger index sits in the EARLIER lane
        vals = np.linspace(-3.0, -1.0, count).astype(np.float32)
        vals[[0, count - 1]] = 5.0                                      # from 65 candidates on: lanes of two waves
        want = S.cand_argmax(vals, idx)
        assert want == int(idx.max())
        st0 = S.state(step=2, pos=9, len=4, eos=want)
        res = fa.op_select_rows(lg, pack(fa, [st0]), form=2, advance=1, n_steps=2, out_cap=6, cand=(vals, idx))
        assert res.launches == (2, 0, 0)
        check_member(res, 0, st0, [want] * 2, 1, 6)
        assert int(res.states["done"][0]) == 1
        if count > 1:                                                   # a single maximum in the last lane the count admits
            vals2 = vals.copy()
            vals2[[0, count - 1]] = (-5.0, 6.0)
            res = fa.op_select_rows(lg, pack(fa, [st0]), form=2, advance=0, n_steps=1, out_cap=6, cand=(vals2, idx))
            check_member(res, 0, st0, [int(idx[count - 1])], 0, 6)


@pytest.mark.parametrize("V,chunk", ((1003, 64), (32000, 32), (40000, 64)))
def test_select_candidates_equal_the_vocabulary_walk(fa, V, chunk):
    """the list built as the lm_head launch builds it (one argmax_last per chunk of rows) selects what form 0 selects on the row"""
    rows = S.tie_rows(V)
    sts = start_states(rows)
    full = fa.op_select_rows(rows, pack(fa, sts), form=0, advance=1, n_steps=1, out_cap=8)
    for b, row in enumerate(rows):
        vals, idx = S.chunk_candidates(row, chunk)
        assert 16 <= len(vals) <= 1023
        res = fa.op_select_rows(row[None], pack(fa, [sts[b]]), form=2, advance=1, n_steps=1, out_cap=8, cand=(vals, idx))
        assert S.state_tuple(res.states[0]) == S.state_tuple(full.states[b]) and (res.out_tokens[0] == full.out_tokens[b]).all(), b
        assert int(res.states["token"][0]) == argmax_last(row)


def batch_case(fa, B, V, seed):
    """logits, start states and samplers of a batch: even members ArgMax on a tie row, odd ones sampled with their own seed,
    temperature and filter"""
    rng = np.random.default_rng(seed)
    lg = (rng.normal(size=(B, V)) * 3.0).astype(np.float32)
    ties = S.tie_rows(V, seed)
    for b in range(0, B, 2):
        lg[b] = ties[(b // 2) % len(ties)]
    sts = start_states(lg, seed)
    samplers, kw = [], []
    for b in range(B):
        if b % 2 == 0:
            samplers.append(None)
            kw.append(None)
        else:
            k = dict(temperature=0.7 + 0.05 * (b % 7), seed=100 + b, draws_done=b % 3)
            k.update(dict(top_p=0.8) if b % 4 == 1 else dict(top_k=7))
            samplers.append(fa.make_sampler(k["temperature"], k["seed"], k["draws_done"], k.get("top_p"), k.get("top_k")))
            kw.append(k)
    return lg, sts, samplers, kw


def same(a, b, ia=slice(None), ib=slice(None)):
    return (a.states[ia].tobytes() == b.states[ib].tobytes() and (a.out_tokens[ia] == b.out_tokens[ib]).all() and (a.kept[ia] == b.kept[ib]).all())


@pytest.mark.parametrize("B,V", ((1, 151), (3, 32000), (8, 151), (8, 32000), (33, 151), (64, 151), (64, 1003)))
def test_select_batch_is_the_single_kernel_per_member(fa, B, V):
    n_steps, cap = 3, 10
    lg, sts, samplers, kw = batch_case(fa, B, V, seed=B + V)
    st = pack(fa, sts)
    batch = fa.op_select_rows(lg, st, form=1, advance=1, n_steps=n_steps, out_cap=cap, samplers=samplers)
    single = fa.op_select_rows(lg, st, form=0, advance=1, n_steps=n_steps, out_cap=cap, samplers=samplers)
    assert batch.launches == (0, n_steps, 0) and single.launches == (B * n_steps, 0, 0)
    for b in range(B):
        assert same(batch, single, b, b), (b, batch.states[b], single.states[b], batch.out_tokens[b], single.out_tokens[b])
        s0 = sts[b]["step"]
        if kw[b] is None:
            check_member(batch, b, sts[b], [argmax_last(lg[b])] * n_steps, 1, cap)
            assert (batch.kept[b] == V).all()
        else:
            toks, kept = fa.op_sample(lg[b], n_steps, return_kept=True, **kw[b])
            check_member(batch, b, sts[b], [int(t) for t in toks], 1, cap)
            assert (batch.out_tokens[b, s0:s0 + n_steps] == toks).all() and (batch.kept[b].astype(np.int64) == kept).all(), b
            assert (kept < V).all()                                     # the filter was on
    # no member sees its neighbours: the members in another order give the same results in that order
    perm = np.roll(np.arange(B)[::-1], 1)
    moved = fa.op_select_rows(lg[perm], st[perm], form=1, advance=1, n_steps=n_steps, out_cap=cap, samplers=[samplers[i] for i in perm])
    for j, b in enumerate(perm):
        assert same(moved, batch, j, b), (j, b)


def test_select_batch_without_advance(fa):
    """advance 0 (the packed prefill's selection): slot `step` is written, nothing moves, and the sampler's stream still does"""
    B, V, cap = 5, 151, 8
    lg, sts, samplers, kw = batch_case(fa, B, V, seed=3)
    res = fa.op_select_rows(lg, pack(fa, sts), form=1, advance=0, n_steps=2, out_cap=cap, samplers=samplers)
    assert res.launches == (0, 2, 0)
    for b in range(B):
        toks = [argmax_last(lg[b])] * 2 if kw[b] is None else [int(t) for t in fa.op_sample(lg[b], 2, **kw[b])]
        st = check_member(res, b, sts[b], toks, 0, cap)
        assert (st["pos"], st["len"], st["step"]) == (sts[b]["pos"], sts[b]["len"], sts[b]["step"])


@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("top_n", (0, 3))
@pytest.mark.parametrize("advance", (0, 1))
def test_logprob_records_in_the_state_forms(fa, form, top_n, advance):
    """slot = step - advance after the selection; a slot at the capacity is not written.  Member 0 ends in the last slot, member 1 starts
    there and runs past it, member 2 starts at 0 and samples."""
    V, cap, n_steps = 151, 6, 2
    rng = np.random.default_rng(17 + top_n)
    lg = (rng.normal(size=(3, V)) * 2.0).astype(np.float32)
    lg[0] = S.tie_rows(V)[1]
    steps = (cap - 2, cap - 1, 0) if advance else (cap - 1, cap, 0)
    sts = [S.state(step=s, pos=3 + b, len=9 + b) for b, s in enumerate(steps)]
    kw = dict(temperature=0.9, seed=4, top_k=5)
    samplers = [None, None, fa.make_sampler(0.9, 4, 0, None, 5)]
    res = fa.op_select_rows(lg, pack(fa, sts), form=form, advance=advance, n_steps=n_steps, out_cap=cap + 3, samplers=samplers, lp_cap=cap, top_n=top_n)
    assert res.launches == ((3 * n_steps, 0, 3 * n_steps) if form == 0 else (0, n_steps, n_steps))
    assert res.records.shape == (3, cap + 1)
    fill_f = np.frombuffer(FILL.tobytes(), np.float32)[0]
    seen_last = seen_cut = False
    for b in range(3):
        toks = [argmax_last(lg[b])] * n_steps if b < 2 else [int(t) for t in fa.op_sample(lg[b], n_steps, **kw)]
        _, _, slots = S.select_run(sts[b], toks, advance, cap + 3)
        want = {}
        for tok, slot in zip(toks, slots):
            if slot < cap:
                want[slot] = tok                                        # (advance 0: the later launch overwrites the slot)
            else:
                seen_cut = seen_cut or slot == cap
        seen_last = seen_last or (cap - 1) in want
        for slot in range(cap + 1):
            rec = res.records[b, slot]
            if slot not in want:
                assert rec.tobytes() == b"\xff" * fa.LOGPROB_REC.itemsize, (b, slot)
                continue
            lp, ids, lps = fa.op_logprobs(lg[b:b + 1], [want[slot]], top_n)
            assert rec["chosen"].tobytes() == lp[0].tobytes(), (b, slot)
            assert (rec["ids"][:top_n] == ids[0]).all() and rec["lps"][:top_n].tobytes() == lps[0].tobytes(), (b, slot)
            assert (rec["ids"][top_n:] == FILL).all() and rec["lps"][top_n:].tobytes() == fill_f.tobytes() * (20 - top_n), (b, slot)
    assert seen_last and seen_cut
