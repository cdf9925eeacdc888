"""CPU part of the fp32 claim of tests/test_gpu_verify_lp.py: in fp32 fl_decode_lookup_lp must return exactly the ids of the plain ruled,
guided loop.  That can only be asked where no row is a near-tie, so -- as test_seeds_keep_the_fp32_margin does for the plain lookup
loop -- the oracle and the restatement check here, before any GPU run, that along the ruled, guided greedy continuation of every chosen
(model, seed, rules, guide) case the top-two gap of every ADJUSTED row stays above that test's bound (imported from its source, not
restated), relative to max(1, the row's largest finite magnitude).  The cases are defined here and imported by the GPU test.

Seeds: of 100, 101, ... the first per model for which the bound holds in all three forms and, for the models of the EOS test, whose
16th output under rules + guide has not come up before (found with this file's own search())."""
import inspect
import re

import numpy as np

import guide_ref as gr
import logit_rules_ref as lr
import synth
import test_gpu_decode_lookup as plain_lookup
import verify_adjust_ref as va
from oracle import oracle

MODELS = ["llama_a", "mistral_a", "qwen2_a", "llama_mha", "llama_d100"]   # (test_gpu_verify.py's)
L, N, CAP = 12, 40, 96
FORMS = ["rules", "guide", "both"]
SEEDS = {"llama_a": 122, "mistral_a": 106, "qwen2_a": 118, "llama_mha": 100, "llama_d100": 100}

# the bound of test_seeds_keep_the_fp32_margin: twice the project's fp32 bar, once for each path
_found = re.search(r"rel\.min\(\) > ([0-9.e-]+)", inspect.getsource(plain_lookup.test_seeds_keep_the_fp32_margin))
assert _found, "test_gpu_decode_lookup.test_seeds_keep_the_fp32_margin no longer asserts 'rel.min() > <bound>': take the bound from where it now stands"
BOUND = float(_found.group(1))


def rules_of(cfg, prompt):
    """what an OpenAI-style request with penalties and a logit_bias installs: keyword arguments of Cache.set_logit_rules"""
    V = cfg["vocab_size"]
    bias = {int(V // 3): 2.0, int(V // 5): -1.0, int(V // 7): float("-inf")}
    return dict(prompt_ids=np.asarray(prompt, np.uint32), logit_bias=bias, repetition_penalty=1.15, frequency_penalty=0.4, presence_penalty=0.3)


def automaton_of(cfg):
    """three states; state s allows the ids j with j % 3 != s and (j // 3) % 5 != 4 -- a little over half the vocabulary -- and
    id j leads to state j % 3: every row of a step is masked in the state its own predecessor chose"""
    V = cfg["vocab_size"]
    j = np.arange(V)
    lists = [j[(j % 3 != s) & ((j // 3) % 5 != 4)] for s in range(3)]
    return gr.Automaton(lists, [lst % 3 for lst in lists])


class Teacher:
    """the host's copy of what a ruled, guided cache holds: the table, the scalars, the automaton and its state"""

    def __init__(self, cfg, prompt, form):
        V = cfg["vocab_size"]
        self.form = form
        self.words = self.bias = self.auto = None
        self.scalars = (1.0, 0.0, 0.0)
        self.state = 0
        if form in ("rules", "both"):
            r = rules_of(cfg, prompt)
            self.words, self.bias = lr.table(V, r["prompt_ids"], (), r["logit_bias"])
            self.scalars = (r["repetition_penalty"], r["frequency_penalty"], r["presence_penalty"])
        if form in ("guide", "both"):
            self.auto = automaton_of(cfg)

    def step_row(self, x, token):
        """the plain loop's step: count the input, adjust and mask the raw row"""
        return self.rows(np.asarray(x, np.float32)[None, :], [token])[0]

    def rows(self, x, ids):
        """a verify step's rows [token, *draft] as the selection reads them (nothing is committed)"""
        st = va.states(self.auto, self.state, ids[1:]) if self.auto is not None else None
        return va.adjust(x, ids, self.words, self.bias, self.scalars, self.auto, st)

    def commit(self, inputs, returned):
        """the inputs of the kept rows are counted, the returned ids move the guide"""
        if self.words is not None:
            self.words = va.count_rows(self.words, inputs, len(inputs))
        if self.auto is not None:
            self.state = self.auto.walk_all(self.state, returned)

    def cut(self, draft):
        """the draft up to the first id the guide cannot reach"""
        if self.auto is None:
            return list(draft)
        s, out = self.state, []
        for t in draft:
            if int(t) not in self.auto.lists[s].tolist():
                break
            out.append(int(t))
            s = self.auto.walk(s, int(t))
        return out


def finite_scale(row):
    f = row[np.isfinite(row)]
    return max(1.0, float(np.abs(f).max())) if f.size else 1.0


def top_two_gap(row):
    s = np.sort(row[~np.isnan(row)])
    return float("inf") if s.size < 2 or s[-2] == -np.inf else float(s[-1] - s[-2])


def oracle_run(name, seed, form, n=N):
    """the oracle's ruled, guided greedy continuation: (first, ids [n], smallest relative top-two gap of the adjusted rows)"""
    cfg = synth.CONFIGS[name]
    om = oracle.OracleModel(cfg, synth.as_f32(synth.synth_weights(cfg)))
    p = synth.prompt_ids(cfg, L, seed=seed)
    oc = om.new_cache(CAP)
    lg = om.forward(oc, p, 0)
    s = np.sort(lg)
    worst = (s[-1] - s[-2]) / max(1.0, float(np.abs(lg).max()))        # the prompt's own token: ArgMax of the raw row (rules come after it)
    first = lr.argmax_last(lg)
    t = Teacher(cfg, p, form)
    tok, out = first, []
    for k in range(n):
        y = t.step_row(om.forward(oc, [tok], L + k), tok)
        worst = min(worst, top_two_gap(y) / finite_scale(y))
        nxt = lr.argmax_last(y)
        t.commit([tok], [nxt])
        out.append(nxt)
        tok = nxt
    return first, np.asarray(out, np.uint32), worst


EOS_MODELS = ["llama_a", "mistral_a", "qwen2_a"]
EOS_AT = 15          # the plain loop looks for an EOS after 16 steps: an EOS that is its 16th output leaves its table well defined


def eos_case(first, ids):
    return ids[EOS_AT] not in ids[:EOS_AT] and ids[EOS_AT] != first


def search(name, start=100, stop=400):
    """the first seed whose three forms all keep the bound (how SEEDS was made)"""
    for seed in range(start, stop):
        runs = [oracle_run(name, seed, form) for form in FORMS]
        if all(r[2] > BOUND for r in runs) and (name not in EOS_MODELS or eos_case(*runs[2][:2])):
            return seed
    return None


def test_the_bound_is_the_plain_lookup_tests():
    assert 0 < BOUND < 1e-2


def test_seeds_keep_the_fp32_margin():
    for name in MODELS:
        for form in FORMS:
            first, ids, worst = oracle_run(name, SEEDS[name], form)
            assert worst > BOUND, (name, form, worst)
            assert len(set(ids.tolist())) >= 8, (name, form)            # penalties and guide leave a continuation worth drafting from
            if form == "both" and name in EOS_MODELS:
                assert eos_case(first, ids), name
