"""The step-state and row-moving op entry points without a GPU: fl_op_select_rows / fl_op_move_rows are exported and declared, their
argument structs have the header's layout, and every refusal comes back with its code and a message before the device is touched."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
NEW = ("fl_op_select_rows", "fl_op_move_rows")
BAD, NO_DEVICE, UNSUPPORTED = -8, -9, -10
MAX_CAND = 1024                                       # kMaxArgmaxCand: the lm_head launch's list holds at most 1023 candidates


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    return fastllm_amd


@pytest.fixture(scope="module")
def L(fa):
    return fa.lib()


def test_new_symbols_are_exported_and_declared(fa, L):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", fa.binding.LIB_PATH], text=True)
    assert set(NEW) <= set(re.findall(r" T (fl_[a-z_0-9]+)", out))
    assert re.search(r"#define\s+FL_ABI_VERSION\s+2\b", hdr) and L.fl_abi_version() == 2      # the change only adds entries
    assert re.search(r"#define\s+FL_MOVE_ROWS_GUARD\s+%d\b" % fa.MOVE_ROWS_GUARD, hdr)


def test_argument_structs_have_the_header_layout(fa):
    """every field of the ctypes mirrors, and of the numpy record of a step state, at the header's offset"""
    b = fa.binding
    lines = ['#include <stddef.h>', '#include "%s"' % HEADER]
    for cname, st in (("fl_select_rows_args", b.FlSelectRowsArgs), ("fl_move_rows_args", b.FlMoveRowsArgs)):
        lines.append('_Static_assert(sizeof(%s) == %d, "sizeof(%s)");' % (cname, C.sizeof(st), cname))
        for name, _ in st._fields_:
            lines.append('_Static_assert(offsetof(%s, %s) == %d, "%s.%s");' % (cname, name, getattr(st, name).offset, cname, name))
    lines.append('_Static_assert(sizeof(fl_step_state) == %d, "fl_step_state");' % fa.STEP_STATE.itemsize)
    for name in fa.STEP_STATE.names:
        lines.append('_Static_assert(offsetof(fl_step_state, %s) == %d, "fl_step_state.%s");' % (name, fa.STEP_STATE.fields[name][1], name))
    assert fa.LOGPROB_REC.itemsize == 4 * (1 + 2 * fa.LOGPROBS_MAX_TOP)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write("\n".join(lines) + "\nint main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", c], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _select_args(fa, form=0, advance=1, n_steps=2, top_n=0, B=2, V=16, out_cap=8, lp_cap=0, step=0, samplers=None, cand=None, **null):
    b = fa.binding
    Ba, Va = max(B, 1), max(V, 1)
    st = np.zeros(Ba, fa.STEP_STATE)
    st["step"], st["eos"] = step, -1
    keep = dict(lg=np.zeros((Ba, Va), np.float32), st=st, so=np.full(Ba * 8, 7, np.uint32), tk=np.full((Ba, max(out_cap, 1)), 7, np.uint32),
                kp=np.full((Ba, max(n_steps, 1)), 7, np.uint32), rc=np.full((Ba, max(lp_cap, 0) + 1, 41), 7, np.uint32), ln=np.full(3, 7, np.int32))
    a = b.FlSelectRowsArgs()
    a.struct_size = C.sizeof(b.FlSelectRowsArgs)
    a.form, a.advance, a.n_steps, a.top_n, a.B, a.V, a.out_cap, a.lp_cap = form, advance, n_steps, top_n, B, V, out_cap, lp_cap
    a.logits, a.states, a.states_out, a.out_tokens, a.kept_out, a.lp_records_out, a.launches_out = (keep[n].ctypes.data for n in ("lg", "st", "so", "tk", "kp", "rc", "ln"))
    if samplers is not None:
        keep["sp"] = (b.FlSampler * Ba)(*samplers)
        a.samplers = C.cast(keep["sp"], C.c_void_p)
    if cand is not None:
        keep["cv"], keep["ci"] = np.zeros(max(len(cand), 1), np.float32), np.asarray(list(cand) or [0], dtype=np.int32)
        a.cand_values, a.cand_indices, a.cand_count = keep["cv"].ctypes.data, keep["ci"].ctypes.data, len(cand)
    for name, v in null.items():
        setattr(a, name, v)
    return a, keep


def test_select_rows_argument_errors(fa, L):
    def rc(**kw):
        a, keep = _select_args(fa, **kw)
        r = L.fl_op_select_rows(C.byref(a))
        if r in (BAD, UNSUPPORTED):
            assert all((keep[n] == 7).all() for n in ("so", "tk", "kp", "rc", "ln")) and L.fl_last_error()      # a refused call writes nothing
        return r

    assert L.fl_op_select_rows(None) == BAD and b"null args" in L.fl_last_error()
    assert rc(struct_size=8) == BAD and b"struct_size" in L.fl_last_error()
    assert rc(form=3) == BAD and rc(form=-1) == BAD and b"form" in L.fl_last_error()
    assert rc(advance=2) == BAD and rc(advance=-1) == BAD and b"advance" in L.fl_last_error()
    for name in ("logits", "states", "states_out", "out_tokens"):
        assert rc(**{name: None}) == BAD and b"null argument" in L.fl_last_error(), name
    assert rc(B=0) == BAD and rc(B=65) == BAD and b"B " in L.fl_last_error()
    assert rc(V=0) == BAD and rc(n_steps=0) == BAD and rc(n_steps=65) == BAD and rc(out_cap=0) == BAD
    # the kernel does not bound out_tokens[step]: the entry does
    assert rc(step=7, n_steps=2, out_cap=8) == BAD and b"exceeds out_cap" in L.fl_last_error()
    assert rc(step=6, n_steps=2, out_cap=8) in (0, NO_DEVICE)
    assert rc(step=5, n_steps=4, advance=0, out_cap=8) == BAD                                # the same rule whatever `advance` is
    assert rc(lp_cap=-1) == BAD and rc(lp_cap=1025) == BAD
    assert rc(lp_cap=4, lp_records_out=None) == BAD and rc(lp_cap=4, top_n=21) == BAD and rc(lp_cap=4, top_n=-1) == BAD
    assert rc(lp_cap=4, top_n=17, V=16) == BAD and b"top_n" in L.fl_last_error()
    bad_sampler = fa.make_sampler(0.8)
    bad_sampler.struct_size = 4
    assert rc(samplers=[fa.make_sampler(0.8), bad_sampler]) == BAD and b"fl_sampler" in L.fl_last_error()
    assert rc(samplers=[fa.make_sampler(0.8), fa.make_sampler(0.8, top_k=-1)]) == BAD
    # form 2: one ArgMax member and 1 .. kMaxArgmaxCand - 1 candidates inside the vocabulary
    assert rc(form=2, B=1, cand=[]) == BAD and b"cand_count" in L.fl_last_error()
    assert rc(form=2, B=1, cand=[0] * MAX_CAND, V=2048) == BAD and b"cand_count" in L.fl_last_error()
    assert rc(form=2, B=1, cand=[0] * (MAX_CAND - 1), V=2048) in (0, NO_DEVICE)
    assert rc(form=2, B=1, cand=[3]) in (0, NO_DEVICE)
    assert rc(form=2, B=2, cand=[3]) == BAD and b"one member" in L.fl_last_error()
    assert rc(form=2, B=1, cand=[3], cand_values=None) == BAD and rc(form=2, B=1, cand=[3], cand_indices=None) == BAD
    assert rc(form=2, B=1, cand=[16]) == BAD and rc(form=2, B=1, cand=[-1]) == BAD and b"cand_indices" in L.fl_last_error()
    assert rc(form=2, B=1, cand=[3], samplers=[fa.make_sampler(0.8)]) == BAD and b"ArgMax" in L.fl_last_error()
    for form, kw in ((0, {}), (1, dict(lp_cap=3, top_n=2)), (0, dict(samplers=[fa.make_sampler(0.0), fa.make_sampler(0.7, top_k=3)]))):
        assert rc(form=form, **kw) in (0, NO_DEVICE), form                                   # well-formed: the device, or the loud "no device"


G = 64


def _move_args(fa, kind, rows=2, h=8, vocab=5, dtype=1, use_state=0, ids=(1, 4), tp=2, Vs=4, n_seq=2, n_slab=1, counts=(2, 1), src_slab=None,
               dst_slab=None, nshards=2, n=3, n_tickets=0, tickets=True, out_words=None, force_kind=None, **null):
    b = fa.binding
    k = fa.MOVE_KINDS[kind]
    a = b.FlMoveRowsArgs()
    a.struct_size = C.sizeof(b.FlMoveRowsArgs)
    a.kind, a.dtype, a.use_state = (k if force_kind is None else force_kind), dtype, use_state
    mx = max
    null.update({n: None for n, v in (('ids', ids), ('counts', counts)) if v is None})
    ids, counts = (1, 4) if ids is None else ids, (2, 1) if counts is None else counts
    T = sum(max(c, 0) for c in counts)
    src_slab = T * max(h, 1) if src_slab is None else src_slab
    dst_slab = max(n_seq, 1) * max(h, 1) if dst_slab is None else dst_slab
    payload = {0: rows * h, 1: rows * h, 2: tp * rows * Vs, 3: n_slab * dst_slab, 4: n, 5: 0}[k]
    words = (nshards if k == 4 else 1) * (payload + 2 * G)
    ns = mx(n_seq, 1)
    keep = dict(table=np.zeros((mx(vocab, 1), mx(h, 1)), np.uint16 if dtype == 1 else np.float32), ids=np.asarray(ids, dtype=np.uint32),
                src=np.zeros(mx(1, tp * rows * Vs, n_slab * src_slab, nshards * n), np.float32), counts=np.asarray(counts, dtype=np.int32),
                u=np.zeros(ns, np.uint32), out=np.full(mx(words, 1) + 8, 7, np.uint32), st=np.full(ns * 8, 7, np.uint32), s0=np.full(ns * 16, 7, np.uint32),
                s1=np.full(ns * 16, 7, np.uint32), tk=np.full(ns * (mx(n_tickets, 0) + G), 7, np.uint32), col=np.full(2 * ns + 2 * G, 7, np.uint32),
                ln=np.full(2, 7, np.int32))
    a.rows, a.h, a.vocab, a.tp, a.Vs, a.n_seq, a.n_slab, a.src_slab, a.dst_slab, a.nshards, a.n, a.n_tickets = rows, h, vocab, tp, Vs, n_seq, n_slab, src_slab, dst_slab, nshards, n, n_tickets
    a.table, a.ids, a.src, a.counts = (keep[x].ctypes.data for x in ("table", "ids", "src", "counts"))
    a.tokens = a.pos = a.len = a.plant_tokens = a.plant_errors = keep["u"].ctypes.data
    a.out_words, a.out = (words if out_words is None else out_words), keep["out"].ctypes.data
    a.states_out, a.ss_init_out, a.ss_out, a.collect_out, a.launches_out = (keep[x].ctypes.data for x in ("st", "s0", "s1", "col", "ln"))
    if tickets:
        a.tickets_out = keep["tk"].ctypes.data
    for name, v in null.items():
        setattr(a, name, v)
    return a, keep


def test_move_rows_argument_errors(fa, L):
    def rc(kind, **kw):
        a, keep = _move_args(fa, kind, **kw)
        r = L.fl_op_move_rows(C.byref(a))
        if r in (BAD, UNSUPPORTED):
            assert all((keep[n] == 7).all() for n in ("out", "st", "s0", "s1", "tk", "col", "ln")) and L.fl_last_error()
        return r

    assert L.fl_op_move_rows(None) == BAD and b"null args" in L.fl_last_error()
    assert rc("embed", struct_size=8) == BAD and b"struct_size" in L.fl_last_error()
    assert rc("embed", force_kind=6) == BAD and rc("embed", force_kind=-1) == BAD and b"kind" in L.fl_last_error()
    for kind in ("embed", "embed_batch"):
        assert rc(kind, table=None) == BAD and rc(kind, ids=None) == BAD and rc(kind, out=None) == BAD
        assert rc(kind, h=12) == UNSUPPORTED and b"multiple of 8" in L.fl_last_error()       # h % 8 (and a fortiori h % 4 -> 4 below)
        assert rc(kind, h=4) == UNSUPPORTED
        assert rc(kind, rows=0, ids=()) == BAD and rc(kind, h=0) == BAD and rc(kind, vocab=0) == BAD and rc(kind, dtype=2) == BAD
        assert rc(kind, ids=(1, 5)) == BAD and b"not below vocab" in L.fl_last_error()
        assert rc(kind, out_words=5) == BAD and b"out_words" in L.fl_last_error()
        assert rc(kind) in (0, NO_DEVICE) and rc(kind, dtype=0) in (0, NO_DEVICE)
    assert rc("embed", use_state=1) == BAD and b"one row" in L.fl_last_error()
    assert rc("embed", use_state=1, rows=1, ids=(3,)) in (0, NO_DEVICE)
    # unshard: [tp][B][Vs] with Vs a multiple of 4
    assert rc("unshard_logits", Vs=6) == UNSUPPORTED and b"multiple of 4" in L.fl_last_error()
    assert rc("unshard_logits", rows=0) == BAD and rc("unshard_logits", tp=0) == BAD and rc("unshard_logits", tp=65) == BAD and rc("unshard_logits", Vs=0) == BAD
    assert rc("unshard_logits", src=None) == BAD and rc("unshard_logits", out=None) == BAD
    assert rc("unshard_logits") in (0, NO_DEVICE)
    # gather_last_rows
    assert rc("gather_last_rows", h=6) == UNSUPPORTED and b"multiple of 4" in L.fl_last_error()           # h % 4
    assert rc("gather_last_rows", h=4) in (0, NO_DEVICE)
    assert rc("gather_last_rows", n_seq=0, counts=()) == BAD and rc("gather_last_rows", n_slab=0) == BAD and rc("gather_last_rows", counts=(2, 0)) == BAD
    assert rc("gather_last_rows", src_slab=23) == BAD and b"slab stride" in L.fl_last_error()             # 3 rows of 8
    assert rc("gather_last_rows", dst_slab=15) == BAD and b"slab stride" in L.fl_last_error()             # 2 members of 8
    assert rc("gather_last_rows", src=None) == BAD and rc("gather_last_rows", counts=None) == BAD
    assert rc("gather_last_rows", n_slab=3, src_slab=30, dst_slab=20) in (0, NO_DEVICE)
    # reduce_shards
    assert rc("reduce_shards", nshards=0) == BAD and b"nshards" in L.fl_last_error()
    assert rc("reduce_shards", nshards=65) == BAD and rc("reduce_shards", n=0) == BAD and rc("reduce_shards", src=None) == BAD
    assert rc("reduce_shards", nshards=1) in (0, NO_DEVICE) and rc("reduce_shards") in (0, NO_DEVICE)
    # packed states: tickets to zero need somewhere to lie
    assert rc("packed_states", n_tickets=3, tickets=False) == BAD and b"null pointer" in L.fl_last_error()
    assert rc("packed_states", n_tickets=0, tickets=False) in (0, NO_DEVICE)
    assert rc("packed_states", n_tickets=3) in (0, NO_DEVICE)
    assert rc("packed_states", n_seq=0) == BAD and rc("packed_states", n_tickets=-1) == BAD and rc("packed_states", n_tickets=4097) == BAD
    for name in ("tokens", "pos", "len", "plant_tokens", "plant_errors", "states_out", "ss_init_out", "ss_out", "collect_out"):
        assert rc("packed_states", **{name: None}) == BAD and b"null argument" in L.fl_last_error(), name


def test_wrappers_reach_the_device_or_fail_loudly(fa):
    """no CPU path behind the wrappers: without a GPU they raise FL_ERR_NO_DEVICE"""
    calls = (lambda: fa.op_select_rows(np.zeros((1, 8), np.float32), np.zeros(1, fa.STEP_STATE)), lambda: fa.op_reduce_shards(np.zeros((2, 4), np.float32)))
    for call in calls:
        if fa.device_count() > 0:
            call()
        else:
            with pytest.raises(fa.FastLLMError) as e:
                call()
            assert e.value.code == NO_DEVICE
