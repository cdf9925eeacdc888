"""Which kernels the prefill, the decode step and the batch step launch -- by name, tag and count -- against a recording
(tests/golden/kernel_selection.json) of the library before the projection planner took over the choice: full width, 2 layers,
lengths on both sides of every selection threshold, under the switch sets the policy tools use.  A refactor of the selection
must reproduce every recorded list exactly.

The one intended difference: a batch step (B >= 17) with FL_GEMM_H4=2 never runs a sliced 128 x 256 launch -- the step is a
captured graph in normal use, and a sliced launch's host-side word set would be baked into it.

Record mode (once per library, the experimental one via FL_LIB_PATH; merges into OUT):
    python tests/test_gpu_kernel_selection.py record OUT.json"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_selection.json")

MODELS = ["mistral-7b", "qwen2-7b", "tinyllama-1.1b"]
TS = [2, 16, 17, 33, 64, 65, 128, 129, 176, 256, 257, 512, 513, 545, 641, 769, 1024, 1025, 1121, 2047]
TP_TS = [17, 129, 257, 513, 1025]
BS = [3, 8, 9, 16, 17, 33, 64]
# tools/policy_boundaries.py's conservative selection
OFF = {"gemm_h4": 0, "gemm_w14": 0, "gemm_rope_4w": 0, "attn_pf32_ks2": 1, "attn_pf32_min_t": 640, "h4_nt": 0, "w14_nt": 0, "skinny_nt": 0,
       "rs_lazy": 0, "gemm_skf": 0, "prefill_dma": 0, "gateup_rowsplit": 0}
SETS = {"default": {}, "off": OFF, "gemm_8p=2": {"gemm_8p": 2}, "gemm_streamk=3": {"gemm_streamk": 3},
        "force_generic_gemm=1": {"force_generic_gemm": 1}, "rs_lazy=0": {"rs_lazy": 0}, "debug_rs_parts=1": {"debug_rs_parts": 1},
        "gemm_h4=2": {"gemm_h4": 2}}
EXP_SETS = {"gemm_skf=2": {"gemm_skf": 2}}


def sets_for(exp):
    return dict(SETS, **EXP_SETS) if exp else SETS


def captured_h4_exception(case_id):
    """The batch-step cases where the planner's 'captured' input changes the recorded selection (no sliced h4 launch)."""
    kind, rest = case_id.split(":", 1)
    if kind != "batch":
        return False
    b, sw = rest.split("/", 1)
    return sw == "gemm_h4=2" and int(b[1:]) >= 17


def experimental_build(fa):
    try:
        fa.tune("experimental", 0)
        return True
    except fa.FastLLMError:
        return False


def apply(fa, switches):
    fa.tune("reload_env", 0)
    for k, v in switches.items():
        fa.tune(k, v)


def profiled(gm, fn):
    gm.profile_begin()
    fn()
    stats = gm.profile_end()
    assert len(stats) < 64, "profile table full: the list would be cut"
    return sorted("%s:%d" % (s["name"], s["launches"]) for s in stats)


def build_model(torch, fa, bench, name, tp=1):
    from fastllm_amd.configs import MODEL_CONFIGS
    cfg = dict(MODEL_CONFIGS[name], num_hidden_layers=2)
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0), seed=3)
    kw = {} if tp == 1 else dict(tp_mode=fa.binding.TP_EMULATED, tp_size=tp)
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16", **kw)
    del wts
    torch.cuda.empty_cache()
    return cfg, gm


def prefill_cases(fa, cfg, gm, prefix, ts, sets):
    """One prefill of T tokens and one decode step on the cache it left, per length and switch set."""
    out = {}
    rs = np.random.RandomState(7)
    ids = {T: rs.randint(0, cfg["vocab_size"], size=T + 1).astype(np.uint32) for T in ts}
    for T in ts:
        for sname, sw in sets.items():
            apply(fa, sw)
            c = gm.new_cache(T + 8)

            def run():
                gm.forward(c, ids[T][:T], 0)
                gm.forward(c, ids[T][T:T + 1], T)
            out["%s:T%d/%s" % (prefix, T, sname)] = profiled(gm, run)
            c.close()
    fa.tune("reload_env", 0)
    return out


def batch_cases(fa, cfg, gm, sets):
    """One step of a batch of B streams (each prefilled with a few tokens first), in the layer form the batch picks."""
    out = {}
    rs = np.random.RandomState(9)
    for B in BS:
        for sname, sw in sets.items():
            apply(fa, sw)
            lens = [3 + i % 5 for i in range(B)]
            caches, toks = [], []
            for n in lens:
                c = gm.new_cache(32)
                toks.append(gm.forward_argmax(c, rs.randint(0, cfg["vocab_size"], size=n).astype(np.uint32), 0))
                caches.append(c)
            batch = fa.Batch(gm, caches)
            out["batch:B%d/%s" % (B, sname)] = profiled(gm, lambda: batch.forward(toks, lens, want_logits=False))
            batch.close()
            for c in caches:
                c.close()
    fa.tune("reload_env", 0)
    return out


def run_group(env, group, exp):
    torch, fa, bench = env
    sets = sets_for(exp)
    if group.startswith("tp"):
        tp = int(group[2:])
        cfg, gm = build_model(torch, fa, bench, "mistral-7b", tp)
        out = prefill_cases(fa, cfg, gm, group, TP_TS, sets)
    elif group == "batch":
        cfg, gm = build_model(torch, fa, bench, "mistral-7b")
        out = batch_cases(fa, cfg, gm, sets)
    else:
        cfg, gm = build_model(torch, fa, bench, group)
        out = prefill_cases(fa, cfg, gm, group, TS, sets)
    gm.close()
    return out


GROUPS = MODELS + ["tp2", "tp4", "batch"]


# ---- the recording: entries ("name[tag]:launches") and lists are stored once each, cases point at lists
def encode(cases_by_lib):
    entries, lists, index = [], [], {}
    eidx = {}
    enc = {}
    for lib, cases in cases_by_lib.items():
        enc[lib] = {}
        for cid, lst in sorted(cases.items()):
            key = tuple(lst)
            if key not in index:
                for e in lst:
                    if e not in eidx:
                        eidx[e] = len(entries)
                        entries.append(e)
                index[key] = len(lists)
                lists.append([eidx[e] for e in lst])
            enc[lib][cid] = index[key]
    return dict(entries=entries, lists=lists, **enc)


def decode(doc, lib):
    return {cid: [doc["entries"][e] for e in doc["lists"][li]] for cid, li in doc[lib].items()}


def golden(lib):
    with open(GOLDEN) as f:
        return decode(json.load(f), lib)


@pytest.fixture(scope="module")
def env():
    import torch
    import fastllm_amd as fa
    import bench
    assert torch.cuda.is_available()
    return torch, fa, bench


@pytest.mark.parametrize("group", GROUPS)
def test_kernel_selection_matches_the_recording(env, group):
    fa = env[1]
    exp = experimental_build(fa)
    lib = "exp" if exp else "default"
    want = {cid: lst for cid, lst in golden(lib).items() if cid.split(":", 1)[0] == (group if group != "batch" else "batch")}
    assert want, "no recorded cases for %s / %s" % (group, lib)
    got = run_group(env, group, exp)
    assert sorted(got) == sorted(want), "case sets differ"
    bad = []
    for cid in sorted(want):
        if captured_h4_exception(cid):
            sliced = [e for e in got[cid] if "[h4," in e and ",sliced" in e]
            if sliced:
                bad.append("%s: a sliced h4 launch in the batch step: %s" % (cid, sliced))
        elif got[cid] != want[cid]:
            bad.append("%s:\n  recorded %s\n  now      %s" % (cid, want[cid], got[cid]))
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "record":
        sys.exit(__doc__)
    import torch
    torch.cuda.is_available()
    import fastllm_amd as fa
    import bench
    e = (torch, fa, bench)
    exp = experimental_build(fa)
    lib = "exp" if exp else "default"
    cases = {}
    for g in GROUPS:
        cases.update(run_group(e, g, exp))
        print("%s / %s: %d cases" % (lib, g, len(cases)), flush=True)
    out = sys.argv[2]
    by_lib = {}
    if os.path.exists(out):
        with open(out) as f:
            doc = json.load(f)
        by_lib = {k: decode(doc, k) for k in ("default", "exp") if k in doc}
    by_lib[lib] = cases
    with open(out, "w") as f:
        json.dump(encode(by_lib), f, separators=(",", ":"))
    # the recording library's batch step with gemm_h4=2 is expected to show sliced h4 launches (the fix makes them go)
    for cid in sorted(cases):
        if captured_h4_exception(cid):
            print("%s: sliced h4 launches %s" % (cid, [x for x in cases[cid] if "[h4," in x and ",sliced" in x]))
    print("recorded %d cases for %s into %s (%d bytes)" % (len(cases), lib, out, os.path.getsize(out)))
