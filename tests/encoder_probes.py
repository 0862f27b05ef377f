"""Exact-weight attention inputs of tests/test_encoder_lengths_gpu.py: packed qkv tensors whose softmax weights are (to 1e-9) 1 / len,
1 or 1 / 2, so that the attention output has a closed form a 16-bit kernel must hit to the last place.  numpy only:
tests/test_encoder_probes.py checks here, without a device, that the fp64 softmax formula on these inputs IS the closed form and that the
weight outside the target keys is negligible — so that no GPU assertion rests on an assumption.

One probe is b = L sequences of padded length L with lens[s] = s + 1 (every length 1 .. L), heads = 2, head width HD in {64, 32}:
qkv [L * L, 3 * heads * HD], row s * L + pos, columns head * HD (Q), hidden + head * HD (K), 2 * hidden + head * HD (V).  Every entry is
0, +-1, +-16 or a V value already rounded to the 16-bit type: exact in bf16, f16 and fp32.  Rows at and behind a sequence's length hold keys
and values like the live ones (a kernel that lets one through changes its result).

C[head] is L distinct random +-1 rows of HD elements.
  uniform   Q = 0, K[j] = C[j], V[j, d] = (d == j % HD): every live key weighs 1 / len, out[q, d] = #{j < len : j % HD == d} / len.
  one-hot   K[j] = C[j], Q[q] = 16 C[t(q)], t(q) = (37 q + 11) % len: key t(q) scores 16 HD / sqrt(HD), every other key at least
            32 / sqrt(HD) less (in fact far less: checked); V Gaussian x 1.5; out[q] = V[t(q)].
  two-hot   h = ceil(len / 2), K[j] = C[j % h], Q[q] = 16 C[t1], t1 = (37 q + 11) % h, t2 = t1 + h: two exactly equal (integer) maxima, the
            second one mostly in a later chunk; out[q] = (V[t1] + V[t2]) / 2 where t2 < len, else V[t1]."""
import numpy as np

HEADS = 2
PROBES = ("uniform", "one-hot", "two-hot")
# The largest softmax weight a one-hot / two-hot query may leave on other keys than its targets (asserted by tests/test_encoder_probes.py for every
# sequence and query).
LEAK = 1e-9


def leak_slack(kind, vmax):
    """What fp32 arithmetic on a one-hot / two-hot probe may differ from the closed form by, absolutely, for V values of at most vmax in magnitude
    (float64 array): 2 LEAK vmax for the leaked weight (out = (1 - e) target + e other) and four spacings of fp32 at vmax — the additive term of
    the project's fp32 protocol — for the accumulator: the matrix pipe sums V[t] * 1.0 and the ~1e-15 leak products of a k-step without IEEE
    rounding, and V[t] can come out one fp32 spacing short.  Nothing next to a unit in the last place of a 16-bit value of ordinary size; it is all
    there is where the targets of a two-hot query cancel (V[t1] = -V[t2]: closed form exactly 0, measured on the bf16 HD = 32 kernel: -2^-24).
    The uniform probe has neither effect: 0."""
    vmax = np.asarray(vmax, np.float64)
    if kind == "uniform":
        return 0.0 * vmax
    return 2.0 * LEAK * vmax + 4.0 * np.spacing(vmax.astype(np.float32)).astype(np.float64)


def bf16_round(x):
    """float32 -> the nearest bf16 value (ties to even), as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def f16_round(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def round_v(x, vdtype):
    """vdtype "bf16": 8 significant bits, and exact in f16 as well (values below 2^-17 lose bits to f16's subnormal grid); "f16": 11 bits"""
    assert vdtype in ("bf16", "f16")
    return f16_round(bf16_round(x)) if vdtype == "bf16" else f16_round(x)


def ulp16(x, dtype):
    """spacing of the 16-bit type `dtype` ("bfloat16" / "float16") at |x|, subnormal range included: float64 array"""
    bits, emin = (7, -126) if dtype == "bfloat16" else (10, -14)
    a = np.abs(np.asarray(x, np.float64))
    e = np.frexp(a)[1] - 1                                  # floor(log2 |x|); frexp(0) = (0, 0)
    e = np.where(a == 0, emin, np.maximum(e, emin))
    return np.ldexp(1.0, e - bits)


def lengths(L):
    return np.arange(1, L + 1, dtype=np.int32)


def sign_rows(L, HD, head, seed):
    """C: L distinct +-1 rows of HD elements, one draw per head"""
    rng = np.random.default_rng([seed, HD, L, head])
    C = rng.integers(0, 2, size=(L, HD)).astype(np.float32) * 2 - 1
    assert len(np.unique(C, axis=0)) == L, "the +-1 key rows must be distinct"
    return C


def targets(kind, L):
    """t1, t2 [L sequences, L queries] (t2 = -1: no second target) of the one-hot / two-hot probe"""
    lens = lengths(L).astype(np.int64)[:, None]
    q = np.arange(L, dtype=np.int64)[None, :]
    if kind == "one-hot":
        return (37 * q + 11) % lens, np.full((L, L), -1, np.int64)
    assert kind == "two-hot"
    h = (lens + 1) // 2
    t1 = (37 * q + 11) % h
    t2 = t1 + h
    return t1, np.where(t2 < lens, t2, -1)


def build(kind, HD, L, vdtype="bf16", seed=0):
    """-> qkv float32 [L * L, 3 * HEADS * HD], lens int32 [L], expected float64 [L, L, HEADS, HD] (rows >= lens[s]: meaningless)"""
    assert kind in PROBES and HD in (64, 32)
    x = np.zeros((L, L, 3, HEADS, HD), np.float32)
    want = np.zeros((L, L, HEADS, HD), np.float64)
    lens = lengths(L)
    j = np.arange(L)
    seqs = np.arange(L)[:, None]
    for head in range(HEADS):
        C = sign_rows(L, HD, head, seed)
        if kind == "uniform":
            x[:, :, 1, head] = C[None]
            x[:, :, 2, head] = (j[:, None] % HD == np.arange(HD)[None, :]).astype(np.float32)[None]
            count = np.maximum(0, (lens[:, None].astype(np.int64) - np.arange(HD)[None, :] + HD - 1) // HD)      # [L, HD]
            want[:, :, head] = (count / lens[:, None].astype(np.float64))[:, None, :]
            continue
        V = round_v(np.random.default_rng([seed, HD, L, head, 7]).standard_normal((L, L, HD), dtype=np.float32) * np.float32(1.5), vdtype)
        x[:, :, 2, head] = V                                                                       # another draw per head and per sequence
        t1, t2 = targets(kind, L)
        x[:, :, 0, head] = np.float32(16) * C[t1]
        if kind == "one-hot":
            x[:, :, 1, head] = C[None]
            want[:, :, head] = V[seqs, t1]
        else:
            h = (lens.astype(np.int64) + 1) // 2
            x[:, :, 1, head] = C[j[None, :] % h[:, None]]
            v1, v2 = V[seqs, t1].astype(np.float64), V[seqs, np.maximum(t2, 0)].astype(np.float64)
            want[:, :, head] = np.where((t2 >= 0)[..., None], (v1 + v2) / 2, v1)
    return x.reshape(L * L, 3 * HEADS * HD), lens, want


def softmax_f64(qkv, lens, HD, t1=None, t2=None):
    """The attention formula in fp64 on a packed qkv, sequence by sequence -> out [b, L, HEADS, HD] and, with target keys t1 / t2 [b, L] given
    (t2 = -1: none), leak [b, HEADS, L]: the softmax weight of every query that falls on other keys than its targets"""
    b = len(lens)
    L = qkv.shape[0] // b
    x = np.asarray(qkv, np.float64).reshape(b, L, 3, HEADS, HD)
    out = np.zeros((b, L, HEADS, HD))
    leak = np.zeros((b, HEADS, L))
    rows = np.arange(L)
    for s in range(b):
        n = int(lens[s])
        for head in range(HEADS):
            q, k, v = x[s, :, 0, head], x[s, :n, 1, head], x[s, :n, 2, head]
            sc = q @ k.T / np.sqrt(HD)
            p = np.exp(sc - sc.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            out[s, :, head] = p @ v
            if t1 is not None:
                p[rows, t1[s]] = 0.0
                two = t2[s] >= 0
                p[rows[two], t2[s][two]] = 0.0
                leak[s, head] = p.sum(axis=1)
    return out, leak
