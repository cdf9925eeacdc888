"""verify_adjust_kernel alone (fl_op_verify_adjust) against the numpy restatement of tests/verify_adjust_ref.py, BIT FOR BIT, in its
three forms (rules only, guide only, both), and rules_count_kernel (fl_op_rules_count) against the same restatement's count.

Shapes: V in {1000, 1003, 2051} -- the odd ones put rows i > 0 off a 16-byte boundary and leave a scalar tail, 2051 gives five id
ranges -- with T in {1, 2, 16}, and one T = 16 case each at V = 32 000 and V = 152 064.

Rules: every id list below is laid over the same table, which holds untouched ids, ids with only the prompt bit, counted ids, a word
at 0x7fffffff and one at 0xffffffff (both stay), finite biases and a -inf bias; rp == 1 and rp != 1; x positive, negative, +0, -0 and
+-inf on counted and uncounted ids.  Guide: a state with one id, one with all V ids, one with the ids on both sides of the range
borders (0, 503, 504, 507, 508, 511, 512, V - 1), a random third; rows in different states; a draft id without an edge, where the
state stays.  The table must come back as it went in: the launch only reads it."""
import numpy as np
import pytest

import guide_ref as gr
import logit_rules_ref as lr
import verify_adjust_ref as va

pytestmark = pytest.mark.gpu
FORMS = ["rules", "guide", "both"]
SAT = 0x7FFFFFFF


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def borders(V):
    return np.unique(np.asarray([0, 503, 504, 507, 508, 511, 512, V - 1]))


def automaton(V):
    rng = np.random.default_rng(V)
    lists = [[V // 2], np.arange(V), borders(V), np.sort(rng.choice(V, V // 3, replace=False))]
    nexts = [1, np.arange(V) % 4, 3, (np.asarray(lists[3]) + 1) % 4]
    return gr.Automaton(lists, nexts)


def special_ids(V):
    """ids whose table word or logit is a special case: (prompt bit only, saturated, saturated + prompt bit, -inf bias, plain counted)"""
    return dict(prompt=V // 2, sat=509, sat_prompt=V - 1, banned=7, counted=512, fresh=503)


def table(V):
    rng = np.random.default_rng(V + 1)
    words, bias = lr.table(V, prompt_ids=rng.choice(V, V // 5, replace=False), output_ids=rng.choice(V, V // 2),
                           logit_bias={int(j): float(v) for j, v in zip(rng.choice(V, 40, replace=False), rng.standard_normal(40) * 3)})
    s = special_ids(V)
    words[s["prompt"]] = lr.PROMPT_BIT
    words[s["sat"]] = SAT
    words[s["sat_prompt"]] = 0xFFFFFFFF
    words[s["counted"]] = 3
    words[s["fresh"]] = 0
    bias[s["banned"]] = -np.inf
    bias[s["fresh"]] = 0.0
    return words, bias


def rows(V, T, seed):
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((T, V))).astype(np.float32)
    s = special_ids(V)
    x[:, 0] = -0.0
    x[:, 1] = 0.0
    x[:, V - 1] = np.float32(2.5)
    x[:, 5::97] = -np.inf
    x[:, 11::193] = np.inf
    x[:, s["banned"]] = np.float32(4.0)                                 # (never +inf under the -inf bias: that sum is NaN)
    x[:, s["prompt"]] = np.float32(-1.25) if T == 1 else np.linspace(-2, 2, T).astype(np.float32)
    x[:, s["fresh"]] = np.float32(1.5)
    x[T // 2, s["counted"]] = -0.0
    x[0, s["sat"]] = np.inf
    return x


def id_lists(V, T):
    """name -> ids [T]: row i's input"""
    s = special_ids(V)
    later = np.full(T, s["counted"], np.uint32)
    later[1:] = [(504 + 3 * i) % V for i in range(1, T)]
    later[-1] = later[0]                                                # the step's token comes again as the last draft (T = 1: itself)
    mixed = np.asarray([s["prompt"], s["sat"], s["sat_prompt"], 0, V - 1, s["banned"], 511, 512, 507, 508, V + 3, s["prompt"], 0, 0, 1003 % V, 1],
                       np.uint32)[:T]
    return {"all equal": np.full(T, s["fresh"], np.uint32), "token again later": later, "special words": mixed}


def check(fa, V, T, form, rp, seed=0):
    auto = automaton(V)
    words, bias = table(V)
    x = rows(V, T, 100 * V + T + seed)
    scal = (rp, 0.25, 0.5)
    for name, ids in id_lists(V, T).items():
        for s0 in range(auto.n_states):
            if form == "rules" and s0 > 0:
                break
            st = va.states(auto, s0, ids[1:])                             # the draft is ids[1:]; an id without an edge leaves the state
            kw_r = dict(words=words, biases=bias, scalars=scal) if form != "guide" else {}
            kw_g = dict(guide=auto.csr(), states=st) if form != "rules" else {}
            got, back = fa.op_verify_adjust(x, ids, **kw_r, **kw_g)
            want = va.adjust(x, ids, words if form != "guide" else None, bias, scal, auto if form != "rules" else None, st)
            for i in range(T):
                bad = np.flatnonzero(gr.bits(got[i]) != gr.bits(want[i]))
                assert bad.size == 0, (V, T, form, rp, name, s0, i, bad[:8], got[i][bad[:8]], want[i][bad[:8]])
            if form != "guide":
                assert np.array_equal(back, words), (V, T, form, name)   # the launch left the table alone
            else:
                assert back is None
    return auto


@pytest.mark.parametrize("form,rp", [("rules", 1.0), ("rules", 1.3), ("guide", 1.0), ("both", 1.0), ("both", 1.3)])   # (no scalars reach "guide")
@pytest.mark.parametrize("T", [1, 2, 16])
@pytest.mark.parametrize("V", [1000, 1003, 2051])
def test_rows_bit_for_bit(fa, V, T, form, rp):
    check(fa, V, T, form, rp)


@pytest.mark.parametrize("V", [32000, 152064])
def test_real_vocabularies(fa, V):
    for form in FORMS:
        check(fa, V, 16, form, 1.3)


def test_the_cases_are_what_they_claim():
    """CPU: the id lists and the automaton hold the cases the header names."""
    for V in (1000, 1003, 2051):
        auto = automaton(V)
        words, _ = table(V)
        s = special_ids(V)
        assert words[s["prompt"]] == lr.PROMPT_BIT and words[s["sat"]] == SAT and words[s["sat_prompt"]] == 0xFFFFFFFF
        assert len(auto.lists[0]) == 1 and len(auto.lists[1]) == V and set(borders(V)) == set(auto.lists[2].tolist())
        ids = id_lists(V, 16)
        assert len(set(ids["all equal"].tolist())) == 1 and ids["token again later"][-1] == ids["token again later"][0]
        # rows in different states, and a draft id without an edge
        st = va.states(auto, 2, ids["special words"][1:])
        assert len(set(st)) >= 3
        assert any(auto.walk(a, int(t)) == a and int(t) not in auto.lists[a].tolist() for a, t in zip(st, ids["special words"][1:]))
        # the restatement itself: the count grows by one per row, the saturated words stay, the table is not touched
        x = rows(V, 16, 1)
        w0 = words.copy()
        y = va.adjust(x, ids["all equal"], words, np.zeros(V, np.float32), (1.0, 1.0, 0.0))
        assert np.array_equal(words, w0)
        assert [float(x[i, s["fresh"]] - y[i, s["fresh"]]) for i in range(16)] == [float(i + 1) for i in range(16)]
        assert va.count_rows(words, [s["sat"], s["sat_prompt"], s["prompt"], s["prompt"], V + 3], 5)[[s["sat"], s["sat_prompt"], s["prompt"]]].tolist() == \
            [SAT, 0xFFFFFFFF, 0x80000002]


@pytest.mark.parametrize("V", [1003, 32000])
def test_rules_count(fa, V):
    words, _ = table(V)
    s = special_ids(V)
    ids = np.asarray([s["fresh"], s["sat"], s["fresh"], s["prompt"], V + 3, s["sat_prompt"], 0, V - 1, s["fresh"], 1, 2, 3, 4, 5, 6, s["prompt"]], np.uint32)
    for n in (0, 1, 3, 16):
        got = fa.op_rules_count(words, ids[:n])
        assert np.array_equal(got, va.count_rows(words, ids, n)), (V, n)
