"""The data flow of attn_fwd_kernel (comorag_amd/csrc/encoder_kernels.hip) replayed in numpy, lane by lane, for the three shapes that ship: 64-wide
heads on 4 waves (two staging passes per chunk), 64-wide heads on 8 waves (one pass), 32-wide heads on 4 waves.  MFMA operand / accumulator layouts
(cmr_device.h: lane l of an A or B operand holds row / column l & 31 and k = 8*(l >> 5) + [0,8); accumulator register r of lane l is row
(r & 3) + 8*(r >> 2) + 4*(l >> 5), column l & 31), the transposed scores, the k-slot permutation that lets the probabilities feed the second MFMA from
the registers they were computed in, K and V row-major in double-buffered LDS (the same thread -> (row, segment) staging for both), V's A operand
through a model of the transposing LDS read (ds_read_b64_tr_b16), masking, the online softmax and the all-padding block.
No GPU: this pins the index arithmetic DESIGN.md §4.6 / §4.10 describe; the kernel itself is tested in tests/test_encoder_fused_gpu.py and
tests/test_encoder_head32_gpu.py."""
import numpy as np

CHUNK = 64
LANE = np.arange(64)


def acc_row(r, lane): return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)


def mma(a, b, c):
    """v_mfma_f32_32x32x16: a, b [64 lanes][8], c [64][16]; D = A B^T added to c in the accumulator layout."""
    A = np.zeros((32, 16)); B = np.zeros((32, 16))
    for e in range(8):
        A[LANE & 31, 8 * (LANE >> 5) + e] = a[:, e]
        B[LANE & 31, 8 * (LANE >> 5) + e] = b[:, e]
    D = A @ B.T
    out = c.copy()
    for r in range(16):
        out[:, r] += D[acc_row(r, LANE), LANE & 31]
    return out


def ds_read_tr16_b64(lds, addr):
    """The transposing read, addr[64] in elements: within a 16-lane group, lane i ADDRESSES row i >> 2, columns 4*(i & 3) .. + 3 of a 4 x 16 block
    (four consecutive elements at its address) and RECEIVES column i of the block, rows 0 .. 3: element r of lane i is what lane 4*r + (i >> 2)
    of its group addressed, at offset i & 3."""
    addressed = lds[addr[:, None] + np.arange(4)]                # [lane][4]: row (i >> 2), columns 4*(i & 3) + [0,4) of the lane's group's block
    i = LANE & 15
    return np.stack([addressed[(LANE & 48) + 4 * r + (i >> 2), i & 3] for r in range(4)], axis=1)


def run_block(qkv, L, length, hidden, head, HD, NW, q0, wave):
    """Rows q0 + 32*wave .. + 31 of one head's output as wave `wave` of the workgroup at query block q0 / (32*NW) computes them."""
    KSTR, VSTR = (72, 88) if HD == 64 else (40, 32)              # LDS row strides, elements
    KS, DTN, SEGS = HD // 16, HD // 32, HD // 8                  # k-steps of QK^T; output tiles of PV; 16-byte segments of a K / V row
    PROWS = NW * 64 // SEGS; PASSES = CHUNK // PROWS             # staging passes of PROWS rows: 2 (HD 64, 4 waves) or 1
    assert (HD, NW, PASSES) in ((64, 4, 2), (64, 8, 1), (32, 4, 1))
    qbase = head * HD; kbase = hidden + head * HD; vbase = 2 * hidden + head * HD
    out = np.full((32, HD), np.nan)
    if q0 >= length:                                             # a block of padding rows only: zeros
        for tid in range(NW * 64):
            row = q0 + (tid >> 1)
            if row < L and wave * 32 <= row - q0 < wave * 32 + 32:
                out[row - q0 - wave * 32, (tid & 1) * (HD // 2): (tid & 1) * (HD // 2) + HD // 2] = 0.0
        return out
    g, c = LANE >> 5, LANE & 31
    qrow = q0 + wave * 32 + c
    qf = np.zeros((KS, 64, 8))
    for ks in range(KS):
        qf[ks] = np.where((qrow < L)[:, None], qkv[np.minimum(qrow, L - 1)[:, None], qbase + ks * 16 + g[:, None] * 8 + np.arange(8)], 0.0)
    o = np.zeros((DTN, 64, 16)); m = np.full(64, -1e30); lsum = np.zeros(64)
    nch = (length + CHUNK - 1) // CHUNK
    sc = 1.4426950408889634 / np.sqrt(HD)
    k_lds = np.full((2, CHUNK * KSTR), np.nan); v_lds = np.full((2, CHUNK * VSTR), np.nan)      # (NaN: whatever is read was staged)

    def stage(ch, buf):                                          # load_chunk + store_chunk: K and V alike, rows behind the sequence's end zeros
        tid = np.arange(NW * 64)
        kr, kseg = tid >> (3 if HD == 64 else 2), tid & (SEGS - 1)
        for h in range(PASSES):
            key = ch * CHUNK + kr + PROWS * h
            src = (np.minimum(key, L - 1)[:, None], kseg[:, None] * 8 + np.arange(8))
            live = (key < length)[:, None]
            k_lds[buf, (kr + PROWS * h)[:, None] * KSTR + kseg[:, None] * 8 + np.arange(8)] = np.where(live, qkv[src[0], kbase + src[1]], 0.0)
            v_lds[buf, (kr + PROWS * h)[:, None] * VSTR + kseg[:, None] * 8 + np.arange(8)] = np.where(live, qkv[src[0], vbase + src[1]], 0.0)

    stage(0, 0)
    for ch in range(nch):
        cur = ch & 1
        s = np.zeros((2, 64, 16))
        for t in range(2):
            for ks in range(KS):
                kf = k_lds[cur][((t * 32 + c) * KSTR + ks * 16 + g * 8)[:, None] + np.arange(8)]
                s[t] = mma(kf, qf[ks], s[t])
        k0 = ch * CHUNK
        if k0 + CHUNK > length:
            for t in range(2):
                for r in range(16):
                    s[t, k0 + t * 32 + acc_row(r, LANE) >= length, r] = -1e30
        cm = s.max(axis=(0, 2))
        cm = np.maximum(cm, cm[LANE ^ 32])
        mn = np.maximum(m, cm)
        alpha = np.exp2((m - mn) * sc)
        p = np.exp2(s * sc - (mn * sc)[None, :, None])
        lsum = lsum * alpha + p.sum(axis=(0, 2)); m = mn
        o *= alpha[None, :, None]
        for t in range(2):
            for sp in range(2):
                pb = p[t][:, 8 * sp: 8 * sp + 8]
                kb = t * 32 + sp * 16 + 4 * g
                for dt in range(DTN):
                    vblk = (kb + ((LANE & 15) >> 2)) * VSTR + dt * 32 + 16 * ((LANE >> 4) & 1) + 4 * (LANE & 3)
                    va = np.concatenate([ds_read_tr16_b64(v_lds[cur], vblk), ds_read_tr16_b64(v_lds[cur], vblk + 8 * VSTR)], axis=1)
                    # the A operand of lane (c, g): V[kb + {0..3, 8..11}][32 dt + c] (zeros behind the sequence's end)
                    keys = k0 + kb[:, None] + np.array([0, 1, 2, 3, 8, 9, 10, 11])
                    assert np.array_equal(va, np.where(keys < length, qkv[np.minimum(keys, L - 1), vbase + 32 * dt + c[:, None]], 0.0))
                    o[dt] = mma(va, pb, o[dt])
        if ch + 1 < nch: stage(ch + 1, cur ^ 1)
    inv = 1.0 / (lsum + lsum[LANE ^ 32])
    for lane in range(64):
        for dt in range(DTN):
            for rr in range(4):
                for j in range(4):
                    out[c[lane], dt * 32 + 8 * rr + 4 * g[lane] + j] = o[dt, lane, 4 * rr + j] * inv[lane]
    return out


# (HD, waves, L, live tokens, (q0, wave) blocks): one padded row of a mini-batch, 2 heads, head 1 checked
CASES = {
    # rows 0-31, 64-95, 96-99 (+ 28 rows past the end of the mini-batch); one chunk of 64 keys and one that ends at key 77
    "hd64_4waves": (64, 4, 100, 77, ((0, 0), (0, 2), (0, 3))),
    # 256 query rows per workgroup, four chunks, the last ends mid-chunk at key 201: rows 0-31, 192-223 (straddling the end), 224-255, and the
    # second workgroup's rows 256-259, a block of padding only
    "hd64_8waves": (64, 8, 260, 201, ((0, 0), (0, 6), (0, 7), (256, 0))),
    "hd32_4waves": (32, 4, 100, 77, ((0, 0), (0, 2), (0, 3))),
}


def test_attention_kernel_data_flow_equals_softmax_attention():
    for case in sorted(CASES):
        _check_case(*CASES[case])


def _check_case(HD, NW, L, length, blocks):
    nh, head = 2, 1
    hidden = nh * HD
    qkv = np.random.default_rng(0).standard_normal((L, 3 * hidden)).astype(np.float32).astype(np.float64)
    Q = qkv[:, head * HD: head * HD + HD]
    K = qkv[:length, hidden + head * HD: hidden + head * HD + HD]
    V = qkv[:length, 2 * hidden + head * HD: 2 * hidden + head * HD + HD]
    S = Q @ K.T / np.sqrt(HD)
    P = np.exp(S - S.max(1, keepdims=True))
    P /= P.sum(1, keepdims=True)
    ref = P @ V
    for q0, wave in blocks:
        got = run_block(qkv, L, length, hidden, head, HD, NW, q0, wave)
        rows = np.arange(q0 + wave * 32, min(q0 + wave * 32 + 32, L))
        if q0 >= length:                               # the kernel writes zeros there (padding rows: nothing reads them but LayerNorm)
            assert np.array_equal(got[:len(rows)], np.zeros((len(rows), HD)))
        else:
            assert np.abs(got[:len(rows)] - ref[rows]).max() < 1e-5
