"""A lane-by-lane NumPy emulation of csrc/dal3_pillars.hip's feature kernel (pillar_feature_kernel and pillar_pack_kernel):
the packed fragment layout, the first layer's k-steps, the accumulators handed on as the second layer's B operand, the
butterfly maxima that leave every lane of a half with its channels' maximum, the per-pillar term and the store pattern,
with dal3_device.h's accumulator layout (column = lane & 31, row = tile_chan(register, lane >> 5)). It models the index
logic and float32 accumulation, not the MFMA's internal rounding. tests/test_pillars_cpu.py holds it to the float64 truth
within the GPU test's bars: a wrong layout or k-step order reads as an error of order one."""
import numpy as np

KS = 7


def tile_chan(r, h): return (r & 3) + 8 * (r >> 2) + 4 * h
def pack(sd, n_layers, C, eps):
    def fold(i):
        p = f"pfn_layers.{i}."
        sc = sd[p+"norm.weight"].astype(np.float64) / np.sqrt(sd[p+"norm.running_var"].astype(np.float64) + eps)
        W = (sd[p+"linear.weight"].astype(np.float64) * sc[:, None]).astype(np.float32)
        b = (sd[p+"norm.bias"].astype(np.float64) - sd[p+"norm.running_mean"].astype(np.float64) * sc).astype(np.float32)
        return W, b
    W1, b1 = fold(0)
    A1 = np.zeros((2, KS, 64), np.float32)
    for mt in range(2):
        for s in range(KS):
            for l in range(64):
                row, col = 32*mt + (l & 31), 2*s + (l >> 5)
                if row < W1.shape[0] and col < W1.shape[1]: A1[mt, s, l] = W1[row, col]
    B1 = np.zeros(64, np.float32); B1[:b1.size] = b1
    A2a = np.zeros((2, 16, 64), np.float32); A2b = np.zeros((2, 16, 64), np.float32); B2 = np.zeros(64, np.float32)
    if n_layers == 2:
        W2, b2 = fold(1); B2[:] = b2
        for mt in range(2):
            for s in range(16):
                for l in range(64):
                    A2a[mt, s, l] = W2[32*mt + (l & 31), tile_chan(s, l >> 5)]
                    A2b[mt, s, l] = W2[32*mt + (l & 31), 32 + tile_chan(s, l >> 5)]
    return A1, B1, A2a, A2b, B2
_L, _R = np.meshgrid(np.arange(64), np.arange(16), indexing="ij")
_ROW, _COL = (_R & 3) + 8 * (_R >> 2) + 4 * (_L >> 5), _L & 31      # the accumulator layout: lane, register -> row, column


def mfma(a, b, c):
    """v_mfma_f32_32x32x2_f32 on (64,) operands and a (64 lanes, 16 registers) accumulator: the two products of a k-step
    summed exactly, one float32 rounding into the accumulator"""
    # a, b: (64,), c: (64,16); C[row][col] += sum_k A[row][k] B[k][col]
    A = np.stack([a[:32], a[32:]], 1).astype(np.float64)   # (32 rows, 2)
    Bm = np.stack([b[:32], b[32:]], 0).astype(np.float64)  # (2, 32 cols)
    D = A @ Bm
    return (c + D[_ROW, _COL]).astype(np.float32)
def tile_from_channels(v):
    t = np.zeros((64, 16), np.float32)
    for l in range(64):
        for r in range(16): t[l, r] = v[tile_chan(r, l >> 5)]
    return t
def max_cols(a):
    out = a.copy()
    for h in range(2):
        out[32*h:32*h+32] = a[32*h:32*h+32].max(0, keepdims=True)
    return out
def kernel(pk, vox, num, co, C, T, n_layers, vx, vy, xo, yo):
    A1, B1, A2a, A2b, B2 = pk
    MT1 = 1 if n_layers == 2 else 2
    NT = 2 if T > 32 else 1
    P = vox.shape[0]; out = np.zeros((P, 64), np.float32)
    f32 = np.float32
    for p in range(P):
        s3 = np.zeros(3, np.float32)
        for r in range(T): s3 = (s3 + vox[p, r, :3]).astype(np.float32)
        mean = s3 / f32(num[p])
        cx = f32(f32(co[p, 3]) * f32(vx)) + f32(xo); cy = f32(f32(co[p, 2]) * f32(vy)) + f32(yo)
        x1 = {}
        for j in range(NT):
            inn = np.zeros((64, KS), np.float32)
            for l in range(64):
                n, h = l & 31, l >> 5
                r = min(32*j + n, T - 1)
                f = np.zeros(8, np.float32); f[:C] = vox[p, r]
                dec = [f[0]-mean[0], f[1]-mean[1], f[2]-mean[2], f[0]-cx, f[1]-cy]
                mask = f32(1 if r < num[p] else 0)
                for s in range(KS):
                    k = 2*s + h; v = f32(0)
                    for d in range(5):
                        if k - C == d: v = dec[d]
                    for c in range(8):
                        if k == c and c < C: v = f[c]
                    inn[l, s] = v * mask
            for mt in range(MT1):
                acc = tile_from_channels(B1[32*mt:32*mt+32])
                for s in range(KS): acc = mfma(A1[mt, s], inn[:, s], acc)
                x1[j, mt] = np.maximum(acc, 0)
        max1 = []
        for mt in range(MT1):
            m = x1[0, mt]
            for j in range(1, NT): m = np.maximum(m, x1[j, mt])
            max1.append(max_cols(m))
        def store(m, mt):
            for l in range(64):
                n, h = l & 31, l >> 5
                if n < 16: out[p, 32*mt + tile_chan(n, h)] = m[l, n]
        if n_layers == 1:
            for mt in range(2): store(max1[mt], mt)
            continue
        for mt in range(2):
            term = tile_from_channels(B2[32*mt:32*mt+32])
            for s in range(16): term = mfma(A2b[mt, s], max1[0][:, s], term)
            best = None
            for j in range(NT):
                acc = term
                for s in range(16): acc = mfma(A2a[mt, s], x1[j, 0][:, s], acc)
                best = acc if best is None else np.maximum(best, acc)
            store(max_cols(np.maximum(best, 0)), mt)
    return out
