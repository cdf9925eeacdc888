"""A numpy float64 decoder forward that returns EVERY row's final hidden state, under the causal mask (candle's sliding-window
rule, App. A.5) or a full one -- the reference of the decoder-model embedding tests (fl_batch_embed).  The project's oracle knows
only the causal mask and returns only last-position logits; tests/test_decoder_ref.py anchors this restatement to it (and to the
golden logits) on the CPU, so that its full-mask output is not trusted blindly.

Embedding, RMSNorm (x / sqrt(mean(x^2) + eps) * w), q/k/v with optional bias, rotate-half RoPE from float32 tables as the library
builds them (inv_freq, the angle and cos / sin all in float32, then widened), GQA attention, SwiGLU."""
import numpy as np


def rope_tables(cfg, n_pos):
    """cos / sin [n_pos, d/2] as build_rope makes them: float32 arithmetic throughout"""
    d = cfg["hidden_size"] // cfg["num_attention_heads"]
    theta = np.float32(cfg.get("rope_theta") or 10000.0)
    j = np.arange(d // 2, dtype=np.float32)
    inv = (np.float32(1.0) / np.power(theta, (np.float32(2.0) * j) / np.float32(d), dtype=np.float32)).astype(np.float32)
    ang = (np.arange(n_pos, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    return np.cos(ang, dtype=np.float32).astype(np.float64), np.sin(ang, dtype=np.float32).astype(np.float64)


def visible(T, mask, window, call0=0):
    """[T, T] bool: may query i see key j.  causal: j <= i and (no window or j + window >= i); full: everything, no window.
    call0 > 0: rows [0, call0) were an earlier call, whose keys a later row sees as an unmasked cached prefix (App. A.5: the window
    runs over a call's own tokens) -- what forwarding [0, call0) and then [call0, T) into one cache computes."""
    if mask == "full":
        return np.ones((T, T), dtype=bool)
    assert mask == "causal"
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    return (j <= i) & ((window is None) | (j + (window or 0) >= i) | ((j < call0) & (i >= call0)))


def rmsnorm(x, w, eps):
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * w


def hidden_states(cfg, weights, ids, mask="causal", pos=0, call0=0):
    """weights: dict name -> float array (HF names).  Returns [T, h] float64: the model's final RMSNorm output of every row.
    call0: see visible()."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items()}
    ids = np.asarray(ids, dtype=np.int64)
    T, h, H = ids.size, cfg["hidden_size"], cfg["num_attention_heads"]
    Hkv = cfg.get("num_key_value_heads") or H
    d, G, eps = h // H, H // Hkv, cfg["rms_norm_eps"]
    window = cfg.get("sliding_window") or None
    cos, sin = rope_tables(cfg, pos + T)
    cos, sin = cos[pos:pos + T, None, :], sin[pos:pos + T, None, :]
    vis = visible(T, mask, window, call0)

    def rope(a):                                         # [T, heads, d], rotate-half
        a1, a2 = a[..., :d // 2], a[..., d // 2:]
        return np.concatenate([a1 * cos - a2 * sin, a2 * cos + a1 * sin], axis=-1)

    x = w["model.embed_tokens.weight"][ids]
    for l in range(cfg["num_hidden_layers"]):
        p = "model.layers.%d." % l
        xn = rmsnorm(x, w[p + "input_layernorm.weight"], eps)
        proj = {}
        for n in "qkv":
            y = xn @ w[p + "self_attn.%s_proj.weight" % n].T
            if p + "self_attn.%s_proj.bias" % n in w:
                y = y + w[p + "self_attn.%s_proj.bias" % n]
            proj[n] = y.reshape(T, -1, d)
        q, k, v = rope(proj["q"]), rope(proj["k"]), proj["v"]
        ao = np.zeros((T, H, d))
        for hq in range(H):
            sc = q[:, hq, :] @ k[:, hq // G, :].T / np.sqrt(d)
            sc = np.where(vis, sc, -np.inf)
            pr = np.exp(sc - sc.max(axis=1, keepdims=True))
            ao[:, hq, :] = (pr / pr.sum(axis=1, keepdims=True)) @ v[:, hq // G, :]
        x = x + ao.reshape(T, H * d) @ w[p + "self_attn.o_proj.weight"].T
        xn = rmsnorm(x, w[p + "post_attention_layernorm.weight"], eps)
        g, u = xn @ w[p + "mlp.gate_proj.weight"].T, xn @ w[p + "mlp.up_proj.weight"].T
        x = x + (g / (1.0 + np.exp(-g)) * u) @ w[p + "mlp.down_proj.weight"].T
    return rmsnorm(x, w["model.norm.weight"], eps)


def logits(cfg, weights, hidden):
    """hidden @ lm_head^T in float64"""
    return np.asarray(hidden, dtype=np.float64) @ np.asarray(weights["lm_head.weight"], dtype=np.float64).T


# ---- the pooling arithmetic of fl_batch_embed, restated in numpy float32 (every operation rounded on its own) ----------------------
def hid_f32(x, inv_rms, w):
    """hid[t][j] = (x[t][j] * inv_rms[t]) * w[j]"""
    x, inv_rms, w = np.asarray(x, np.float32), np.asarray(inv_rms, np.float32), np.asarray(w, np.float32)
    return ((x * inv_rms[:, None]).astype(np.float32) * w[None, :]).astype(np.float32)


def pool_f32(hid, counts, pooling, dims=0):
    """unnormalised pooled vectors [n, dims] (pooling 'none': [T, dims]) of the rows hid [T, h], members of counts[i] rows"""
    hid = np.asarray(hid, np.float32)
    dims = dims or hid.shape[1]
    if pooling == "none":
        return hid[:, :dims].copy()
    out, r = [], 0
    for c in counts:
        rows = hid[r:r + c, :dims]
        if pooling == "last":
            out.append(rows[-1])
        elif pooling == "first":
            out.append(rows[0])
        else:
            acc = np.zeros(dims, np.float32)
            for t in range(c):
                acc = (acc + rows[t]).astype(np.float32)
            out.append((acc / np.float32(c)).astype(np.float32))
        r += c
    return np.stack(out)


def normalize_f64(p):
    """the exact normalisation of fp32 vectors p [n, dims]; a zero vector stays zero"""
    p = np.asarray(p, np.float64)
    n = np.sqrt((p * p).sum(axis=1, keepdims=True))
    return np.where(n > 0, p / np.where(n > 0, n, 1.0), 0.0)


def check_normalized(got, p, what=""):
    """got against the float64 normalisation of the exact fp32 vectors p: relative error <= 2 * dims * 2^-24 -- the first-order worst
    case of any fp32 summation order over dims non-negative terms, doubled for the square root and the division (derived, not
    measured)."""
    want = normalize_f64(p)
    dims = want.shape[1]
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - want)
    lim = 2.0 * dims * 2.0 ** -24 * np.abs(want)
    assert (err <= lim).all(), "%s: worst err / bound %.3g" % (what, float((err / np.maximum(lim, 1e-300)).max()))
