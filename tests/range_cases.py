"""Inputs, host models and bounds of the dynamic-range tests (tests/test_range_host.py on the CPU,
tests/test_gpu_dynamic_range.py on the device).  Nothing here touches a GPU.

The operand formats ("numeric range contract"):
  bf16 pair   hi = RNE_bf16(v), lo = RNE_bf16(v - hi): |hi + lo - v| <= 2^-17 |v|  (2^-9 of 2^-9, and a factor 2 to spare)
              while both halves are normal bf16 numbers, |v| in [2^-100, 2^100] here;
  bf16 triple h, m = RNE(v - h), l = RNE(v - h - m): h + m + l == v exactly (3 x 8 significand bits cover fp32's 24);
  fp16 pair   hi = RTZ_fp16(v), lo = RTZ_fp16(v - hi): 2^-20 |v| while lo is a normal fp16 number; below that the pair is a
              fixed-point number with quantum 2^-24 (the fp16 subnormal spacing); |v| < 65504 or hi saturates."""

import math

import numpy as np
import torch

LOG2E = 1.4426950408889634
RANGE_LO, RANGE_HI = 2.0 ** -100, 2.0 ** 100          # no input, product or K-sum of a test may leave this


# ------------------------------------------------------------------------------------------------------------ host models
def bf16_rne_bits(v):
    """fp32 array -> its bf16 bit pattern (uint16), round to nearest even: u += 0x7FFF + ((u >> 16) & 1), as the kernels do."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF
    return (u >> 16).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split_bf16(v):
    """(hi, lo) fp32 arrays holding bf16 values: the split of split2 / split3 / split2_weight."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    hi = bf16_value(bf16_rne_bits(v))
    lo = bf16_value(bf16_rne_bits(v - hi))
    return hi, lo


def split3_bf16(v):
    """(h, m, l): the three planes of x6_pack."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    h = bf16_value(bf16_rne_bits(v))
    m = bf16_value(bf16_rne_bits(v - h))
    l = bf16_value(bf16_rne_bits((v - h) - m))
    return h, m, l


def fp16_rtz(v):
    """fp32 array -> fp16 array, round toward zero (v_cvt_pkrtz_f16_f32), subnormal results kept; |v| < 65504."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    with np.errstate(over='ignore'):
        h = v.astype(np.float16)                                     # round to nearest even ...
    away = np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64))
    h = np.where(away, np.nextafter(h, np.float16(0)), h)            # ... one step back where that went away from zero
    return h.astype(np.float16)


def split_fp16(v):
    """(hi, lo) fp16 arrays: the attention operand image of linear_x3_qkv / ln_qkv_fused."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    hi = fp16_rtz(v)
    lo = fp16_rtz(v - hi.astype(np.float32))
    return hi, lo


E_H_FLOOR = 2.0 ** -24


def e_bf(v):
    """Representation bound of the bf16 pair."""
    return 2.0 ** -17 * np.abs(np.asarray(v, dtype=np.float64))


def e_h(v):
    """Representation bound of the fp16 pair: 2^-20 relative, never below the fixed-point quantum 2^-24."""
    return np.maximum(2.0 ** -20 * np.abs(np.asarray(v, dtype=np.float64)), E_H_FLOOR)


# ------------------------------------------------------------------------------------------------------------ section 2
SPLIT_EXPONENTS = tuple(range(-100, 101, 10))
SPLIT_SHAPES = tuple((r, c) for r in (1, 33, 129) for c in (32, 256))


def split_values(rows, channels, seed):
    """+-m 2^e with a random 24-bit m (the top bit set: every value uses all 24 significand bits it can) and e cycling over
    SPLIT_EXPONENTS element by element; the mantissa is normalised so that |v| lies in [2^e, 2^(e+1)) for e < 0 and in
    [2^(e-1), 2^e) for e >= 0: inside [2^-100, 2^100]."""
    rs = np.random.RandomState(seed)
    n = rows * channels
    m = rs.randint(1 << 23, 1 << 24, size=n).astype(np.float64)
    e = np.array(SPLIT_EXPONENTS, dtype=np.int64)[(np.arange(n) + rs.randint(0, 1000)) % len(SPLIT_EXPONENTS)]
    sign = np.where(rs.randint(0, 2, size=n) == 1, -1.0, 1.0)
    v = sign * np.ldexp(m, np.where(e < 0, e - 23, e - 24))
    out = v.astype(np.float32)
    assert (out.astype(np.float64) == v).all()
    return torch.from_numpy(out.reshape(rows, channels))


def shrink_exponents(t):
    """The same significands with the binary exponents shrunk to 9/10: 2^-100 .. 2^100 becomes 2^-90 .. 2^90."""
    m, e = torch.frexp(t)
    return torch.ldexp(m, torch.div(e * 9, 10, rounding_mode='trunc'))


def row_scales(rows, seed):
    """Per-row factors of split2(row_scale=): stochastic-depth style (0, 1 / keep) and powers of two."""
    rs = np.random.RandomState(seed)
    pool = np.array([0.0, 1.0, 1.0 / 0.9, 2.0 ** -12, 2.0 ** 12, 1.25], dtype=np.float32)
    return torch.from_numpy(pool[rs.randint(0, len(pool), size=rows)])


# ------------------------------------------------------------------------------------------------------------ sections 3, 4
SCALES_A = (-40, -16, 0, 16, 40)
SCALES_B = (-20, 0, 20)
ERR_SCALES = (-16, 0, 16)
COLUMN_SHIFT = 12                                     # per-column exponents a_k in [-12, 12]
GEMM_M = (1, 127, 129)
GEMM_KN = ((32, 128), (96, 384), (256, 128))          # the smallest pair the predicates accept (K % 32, N % 128) and larger
WGRAD_M = (1, 31, 33, 1000)
WGRAD_NK = ((128, 128), (256, 384))                   # the smallest pair (N % 128, K % 128) and one larger
X6_TILES = (0, 2, 4, 12, 14)                          # the tile shapes test_linear_x6_planes_are_exact_and_layout walks
MAG_LO, MAG_HI = 2.0 ** -10, 8.0                      # magnitudes of the GEMM data before scaling
C_X3 = 2.0 ** -15
C_X6_FLOOR = 2.0 ** -22


def real_values(shape, seed, sigma=1.0):
    """sigma * randn with the magnitudes clamped into [2^-10, 8]: real-valued data whose products stay representable."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(*shape, generator=g) * sigma
    mag = r.abs().clamp(MAG_LO, MAG_HI)
    return torch.where(r < 0, -mag, mag)


def gemm_case(m, k, n, seed):
    """x (m, k), w (n, k), bias (n), residual (m, n)."""
    return (real_values((m, k), seed), real_values((n, k), seed + 1, 0.25), real_values((n,), seed + 2, 0.5),
            real_values((m, n), seed + 3, 2.0))


def pow2(t, e):
    """t * 2^e, exactly."""
    return torch.ldexp(t, torch.tensor(e))


def column_exponents(k, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(-COLUMN_SHIFT, COLUMN_SHIFT + 1, size=k).astype(np.int32))


def grouped_tiles(sizes, npad, tile_rows=128):
    """(tiles [(first row, rows, first weight row)], edges) of a grouped launch with sizes[k] rows on weight block k."""
    edges = [0]
    for s in sizes:
        edges.append(edges[-1] + s)
    tiles = [(a, min(tile_rows, edges[b + 1] - a), b * npad) for b in range(len(sizes))
             for a in range(edges[b], edges[b + 1], tile_rows)]
    return tiles, edges


GROUP_SIZES = (0, 1, 127, 129, 33)
GROUP_KN = ((32, 64), (64, 128), (128, 256))


# ------------------------------------------------------------------------------------------------------------ GELU sweep
def gelu_sweep():
    """v = j 2^-7 for |j| < 2^15 (|v| < 256), then +-0, +-2^-20, +-300: every value has at most 16 significant bits, so a bf16
    pair holds it exactly and an identity weight hands it to the epilogue unchanged."""
    j = np.arange(-(1 << 15) + 1, 1 << 15, dtype=np.float64)
    extra = np.array([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 300.0, -300.0])
    return torch.from_numpy(np.concatenate([j * 2.0 ** -7, extra]).astype(np.float32))


def gelu_random(n=4096, seed=7):
    """fp32 values in [-12, 12] with full mantissas (for the x6 epilogues, whose three planes hold any fp32 value)."""
    return torch.from_numpy(np.random.RandomState(seed).uniform(-12.0, 12.0, size=n).astype(np.float32))


def gelu64(v):
    v = v.double()
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def gelu_grad64(v):
    v = v.double()
    return 0.5 * (1.0 + torch.erf(v * math.sqrt(0.5))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


ERF_ABS = 1.5e-7                                      # Abramowitz & Stegun 7.1.26


def gelu_format_bound(v):
    """0.5 |v| 1.5e-7 (the erf approximation, multiplied by v / 2) + 2^-24."""
    return 0.5 * v.double().abs() * ERF_ABS + 2.0 ** -24


def gelu_grad_format_bound(v):
    """d/dv gelu = Phi(v) + v phi(v): the erf error enters Phi without the factor v, 0.5 * 1.5e-7; |v phi(v)| <= 0.242 is
    rounded to fp32 (below 2^-25) and the sum once more (2^-24 at values up to 1.13): + 2^-24, as for the forward."""
    return torch.full_like(v.double(), 0.5 * ERF_ABS + 2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------ LayerNorm rows
LN_SHAPES = ((33, 128), (129, 256))
LN_EPS = 1e-5
LN_CONSTANTS = (3.0, -0.75, 1.3125 * 2.0 ** 14, 1.5 * 2.0 ** -30)     # short significands: every partial sum of a row is exact


def ln_rows(rows, c, seed):
    """(x (rows, c) fp32, kind per row): mean 2^k / std 1 for k in {0, 8, 14}; unit rows times 2^+-30; constant rows; one row
    with a single element 2^20 times the rest."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, c, generator=g)
    kinds = []
    menu = ['mean0', 'mean8', 'mean14', 'up30', 'down30', 'const', 'unit']
    for r in range(rows):
        kind = 'outlier' if r == rows - 1 else menu[r % len(menu)]
        if kind.startswith('mean'):
            x[r] += 2.0 ** int(kind[4:])
        elif kind == 'up30':
            x[r] *= 2.0 ** 30
        elif kind == 'down30':
            x[r] *= 2.0 ** -30
        elif kind == 'const':
            x[r] = LN_CONSTANTS[(r // len(menu)) % len(LN_CONSTANTS)]
        elif kind == 'outlier':
            x[r, (7 * r) % c] *= 2.0 ** 20
        kinds.append(kind)
    return x, kinds


def ln_params(c, seed):
    g = torch.Generator().manual_seed(seed)
    return 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)


def ln64(x, gamma, beta, eps=LN_EPS):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


LN_FLOOR = 2.0 ** -22


# ------------------------------------------------------------------------------------------------------------ attention operands
F16_SCALES = (-20, -14, -8, -3, 0, 8, 15)
F16_MAX = 65504.0
IMAGE_ROWS, IMAGE_C = 129, 128                         # linear_x3_qkv takes C % 128 == 0
IMAGE_AMP = 1.9                                        # |value| <= 1.9: 1.9 * 2^15 < 65504


def image_values(rows, c, seed):
    """Values in [-1.9, 1.9] with full fp32 mantissas and magnitudes spread over 12 binades."""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-IMAGE_AMP, IMAGE_AMP, size=(rows, c)) * np.exp2(-rs.randint(0, 12, size=(rows, c)).astype(np.float64))
    return torch.from_numpy(v.astype(np.float32))


def block_identity_qkv(c):
    """(3c, c) weight whose q, k and v blocks are the identity."""
    return torch.eye(c).repeat(3, 1).contiguous()


def decode_f16_image(buf, rows, heads):
    """Opaque (rows, 3C) float32 buffer -> (hi, lo) fp16 arrays (rows, 3, H, 16)."""
    h = buf.cpu().contiguous().view(torch.float16).reshape(rows, 3, heads, 2, 16).numpy()
    return h[:, :, :, 0], h[:, :, :, 1]


ATT_FAMILIES = ((48, 1, 4), (64, 0, 5))                # (K, G, depth), dilation 1
ATT_H = 2
ATT_SV = (-10, 0, 10)
ATT_SQK = ((0, 0), (4, -4), (-4, 4))
ATT_F32_BOUND = 2.0 ** -20


def logit_bound(q_max, k_max):
    """d_s: what the two fp16 pairs can move a 16-term logit."""
    return 16.0 * (q_max * float(e_h(k_max)) + k_max * float(e_h(q_max)))


def in_range(t):
    """Every non-zero magnitude of t inside [2^-100, 2^100]."""
    a = t.double().abs()
    a = a[a > 0]
    return a.numel() == 0 or (float(a.min()) >= RANGE_LO and float(a.max()) <= RANGE_HI)
