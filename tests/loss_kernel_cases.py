"""Cases and float64 references for the element-by-element tests of the two loss kernels of `csrc/loss.hip`
(`hfl_smoothap_rows`, `hfl_kd_rows`): tests/test_loss_kernel_host.py proves them on the CPU, tests/test_gpu_loss_kernels.py
holds the kernels to them.  Everything is closed-form from a seed (`hotformerloc_amd.synthetic.hash_uniform`), runs on
whatever device the tensors are on, and imports nothing from `oracle/`.

The references restate the formulas of the reference's training step, not the kernels: `smoothap_ref` is the (rows, P, B)
tensor algebra of `models/losses/truncated_smoothap.py:46-93` with the clamped sigmoid of `models/losses/loss_utils.py:40-48`,
differentiated by `torch.autograd`; `kd_ref` is `models/losses/loss.py:138-147` through `log_softmax`.  Both start from the
float32 operands the kernel receives -- the temperature among them: the C ABI takes `tau` and `T` as float, so the references
use the float32 value of either.

The yardstick ("Numeric range contract"): per row, `bar = 2 E32 + 2^-22 scale`, E32 the largest error over the row
of the same formula run in float32 torch, `scale` the float64 sum of the magnitudes of the terms the result is made of."""

import collections

import numpy as np
import torch

from hotformerloc_amd import synthetic as syn

CLAMP = 50.0                      # loss_utils.py:44
CHUNK = 256                       # rows per (rows, P, B) block of the reference
FLOOR = 2.0 ** -22                # of `scale`, per row
LDS_SIZES = ((5461, 2), (5462, 2), (7282, 2), (17066, 1))     # 9 B = 49149 | 49158 (48 KiB = 49152) | 65538 (64 KiB) | 153594
CAPACITY = 17066                  # 9 B <= 150 KiB
TAU = 0.01                        # tau1 of every shipped config


def f32(v) -> float:
    """the value a `float` argument of the C ABI carries"""
    return float(np.float32(v))


def uniform(seed, *shape):
    return syn.hash_uniform(seed, int(np.prod(shape))).reshape(shape)


# ================================================================================================ SmoothAP: reference
SmoothAPRef = collections.namedtuple('SmoothAPRef', 'ap grad scale')


def smoothap_ref(S, pos, neg, idx, tau, dtype=torch.float64, variant=None):
    """Rows of the ranking algebra.  S: (R, B) similarities of R query rows (any float dtype, used as `dtype`), pos / neg:
    (R, B) masks (non-zero = set), idx: (R, P) int64 selected positives.  A slot is valid iff 0 <= idx < B and it points at a
    positive; invalid slots contribute nothing; a row without a valid slot has AP 0 and a zero gradient row.

    Returns (ap (R,), grad (R, B) = d ap_q / d S_q., scale (R,)): `scale` is sum_j sum_z |d ap_q / d e_jz| / tau, e_jz the
    sigmoid's exponent -(s_z - s_pj) / tau -- every entry of the gradient row is a signed sum of those terms.

    `variant` names a deliberately wrong formula (negative controls): 'keep_self' (the own position z == p_j stays in r_p),
    'over_p' (1 / P instead of 1 / n_valid), 'neg_in_rp' (negatives counted in r_p)."""
    tau = f32(tau)
    B, P = S.shape[1], idx.shape[1]
    aps, grads, scales = [], [], []
    for r0 in range(0, S.shape[0], CHUNK):
        s = S[r0:r0 + CHUNK].detach().to(dtype).clone().requires_grad_()
        p = (pos[r0:r0 + CHUNK] != 0)
        n = (neg[r0:r0 + CHUNK] != 0)
        ix = idx[r0:r0 + CHUNK]
        inside = (ix >= 0) & (ix < B)
        ixc = ix.clamp(0, B - 1)
        valid = inside & p.gather(1, ixc)                                    # truncated_smoothap.py:85
        e = -(s.unsqueeze(1) - s.gather(1, ixc).unsqueeze(2)) / tau          # :46, loss_utils.py:43
        a = 1.0 / (1.0 + torch.exp(torch.clamp(e, min=-CLAMP, max=CLAMP)))   # loss_utils.py:44-45
        pa = a * p.unsqueeze(1).to(dtype)                                    # :51-52
        if variant != 'keep_self':
            pa = pa * torch.ones_like(pa).scatter(2, ixc.unsqueeze(2), 0.)   # :55-56
        na = (a * n.unsqueeze(1).to(dtype)).sum(2)
        r_p = pa.sum(2) + 1.0                                                # :59
        if variant == 'neg_in_rp':
            r_p = r_p + na
        r = r_p / (r_p + na)                                                 # :66-69
        n_valid = valid.sum(1)
        denom = torch.full_like(n_valid, P) if variant == 'over_p' else n_valid.clamp(min=1)
        ap = (r * valid.to(dtype)).sum(1) / denom.to(dtype)                  # :86-93, row by row
        g_s, g_e = torch.autograd.grad(ap.sum(), [s, e])
        aps.append(ap.detach())
        grads.append(g_s)
        scales.append(g_e.abs().sum((1, 2)) / tau)
    return SmoothAPRef(torch.cat(aps), torch.cat(grads), torch.cat(scales))


def smoothap_ref64(S, pos, neg, idx, tau):
    r = smoothap_ref(S, pos, neg, idx, tau, torch.float64)
    return r.ap, r.grad


def smoothap_ref32(S, pos, neg, idx, tau):
    r = smoothap_ref(S, pos, neg, idx, tau, torch.float32)
    return r.ap, r.grad


def top_positives(S, pos, P, chunk=1024):
    """The P most similar positives of every row, in float64 (`torch.topk` as truncated_smoothap.py:36-39); slots beyond the
    row length (P > B) hold -1.  Rows with fewer than P positives get indices of non-positives in their spare slots, as the
    reference does."""
    B = S.shape[1]
    k = min(P, B)
    out = torch.full((S.shape[0], P), -1, dtype=torch.int64, device=S.device)
    for r0 in range(0, S.shape[0], chunk):
        sp = S[r0:r0 + chunk].double().masked_fill(pos[r0:r0 + chunk] == 0, float('-inf'))
        out[r0:r0 + chunk, :k] = torch.topk(sp, k=k, dim=1, largest=True, sorted=True)[1]
    return out


SmoothAPCase = collections.namedtuple('SmoothAPCase', 'S pos neg idx tau')


def _case(S, pos, neg, idx, tau):
    return SmoothAPCase(torch.as_tensor(S, dtype=torch.float32).contiguous(), torch.as_tensor(pos).to(torch.uint8).contiguous(),
                        torch.as_tensor(neg).to(torch.uint8).contiguous(), idx.contiguous(), tau)


# ================================================================================================ SmoothAP: cases
SIZES_B = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)
SIZES_P = (1, 2, 4, 7)
TAUS = (0.01, 0.1, 1.0)


def _random_parts(B, seed):
    """S uniform in (-1, 1); about 10 % positives and 60 % negatives, disjoint; the query itself is neither.  At B <= 3 such
    masks are empty and nothing but the zero paths would run: there half of the elements are positives and 60 % negatives,
    independently, the diagonal included (the kernel attaches no meaning to z == q), and row 0 has the positive B - 1 and the
    negative 0 (one element that is both at B = 1)."""
    S = uniform(seed, B, B).astype(np.float32)
    if B <= 3:
        pos, neg = uniform(seed + 1, B, B) < 0.0, uniform(seed + 2, B, B) < 0.2
        pos[0, B - 1], neg[0, 0] = True, True
        return S, pos, neg
    pos = uniform(seed + 1, B, B) < -0.8
    neg = (uniform(seed + 2, B, B) < 1.0 / 3.0) & ~pos
    np.fill_diagonal(pos, False)
    np.fill_diagonal(neg, False)
    return S, pos, neg


def smoothap_random(B, P, tau=TAU, seed=None):
    seed = 1000 * B + 7 if seed is None else seed
    S, pos, neg = (torch.from_numpy(v) for v in _random_parts(B, seed))
    return _case(S, pos, neg, top_positives(S, pos, P), tau)


FAMILY_B, FAMILY_P = 257, 4
FAMILY_ROWS = {'no_pos': 3, 'few_nonpos': 17, 'few_minus1': 18, 'few_b': 19, 'few_b1000': 20, 'few_wrap': 21, 'no_neg': 40,
               'all_pos': 41, 'both': 42, 'diag': 43, 'dup': 44}
FEW_ROWS = ('few_nonpos', 'few_minus1', 'few_b', 'few_b1000', 'few_wrap')
FEW_SPARE = {'few_minus1': -1, 'few_b': FAMILY_B, 'few_b1000': FAMILY_B + 1000}
WRAP = 2 ** 32                   # 'few_wrap': the spare slots hold 2^32 + (index of the best positive), which is not that index


def smoothap_families(tau=TAU):
    """One batch of B = 257, P = 4 whose rows FAMILY_ROWS hold one mask family each; every other row is a random row."""
    B, P = FAMILY_B, FAMILY_P
    S, pos, neg = _random_parts(B, 4242)
    R = FAMILY_ROWS
    pos[R['no_pos'], :] = False
    for k, name in enumerate(FEW_ROWS):                      # exactly two positives
        q = R[name]
        pos[q, :] = False
        pos[q, [(q + 5 + k) % B, (q + 131 + k) % B]] = True
        neg[q, [(q + 5 + k) % B, (q + 131 + k) % B]] = False
    neg[R['no_neg'], :] = False
    pos[R['all_pos'], :] = True                              # the diagonal and the negatives among them
    q = R['diag']
    pos[q, q], neg[q, q], S[q, q] = True, False, 1.0         # the most similar element of its row: selected first
    S, pos, neg = torch.from_numpy(S), torch.from_numpy(pos), torch.from_numpy(neg)
    idx = top_positives(S, pos, P)
    q = R['both']                                            # an unselected positive just below the last selected one, also a negative
    z = int(((pos[q] != 0) & ~torch.isin(torch.arange(B), idx[q])).nonzero()[0])
    S[q, z] = S[q, idx[q, P - 1]] - 0.003
    neg[q, z] = True
    idx = top_positives(S, pos, P)
    assert z not in idx[q].tolist()
    q = R['few_nonpos']
    nonpos = (pos[q] == 0).nonzero().flatten()
    idx[q, 2:] = nonpos[[7, 100]]
    for name, spare in FEW_SPARE.items():
        idx[R[name], 2:] = spare
    idx[R['few_wrap'], 2:] = WRAP + idx[R['few_wrap'], 0]
    q = R['dup']
    idx[q] = idx[q, [0, 0, 1, 2]]
    return _case(S, pos, neg, idx, tau)


def alone(case, q):
    """The batch of `case` with every row but q emptied: zero similarities, no masks, no selected positive."""
    S, pos, neg = torch.zeros_like(case.S), torch.zeros_like(case.pos), torch.zeros_like(case.neg)
    idx = torch.full_like(case.idx, -1)
    S[q], pos[q], neg[q], idx[q] = case.S[q], case.pos[q], case.neg[q], case.idx[q]
    return SmoothAPCase(S, pos, neg, idx, case.tau)


CLAMP_B, CLAMP_TAU = 65, 2.0 ** -6
CLAMP_BASES = (0.0, 0.5, -0.25)                               # s_p of row q: CLAMP_BASES[q % 3]


def clamp_exponents():
    """The exponents e = -(s_z - s_p) / tau a clamp row is built around: exactly -+50, -+50 (1 -+ 2^-20), -+200, -+1e6.
    50 (1 +- 2^-20) needs 25 significand bits; its float32 neighbour is 50 +- 3 * 2^-16 (a tie, rounded to even), which keeps
    s_p - e tau a float32 number for every s_p of CLAMP_BASES."""
    near = [float(np.float32(50.0 * (1 + 2.0 ** -20))), float(np.float32(50.0 * (1 - 2.0 ** -20)))]
    assert near == [50.0 + 3 * 2.0 ** -16, 50.0 - 3 * 2.0 ** -16]
    mags = [50.0] + near + [200.0, 1e6]
    return [s * m for m in mags for s in (1.0, -1.0)]


def smoothap_clamp():
    """B = 65, P = 2, tau = 2^-6.  Row q: slot 0 selects p0 = (q + 1) % B with s_p0 = CLAMP_BASES[q % 3]; ten columns hold
    s_p0 - e tau for the exponents of `clamp_exponents`, the others for e = k 2^-10 in (-8, 8); every such s is a float32
    number and s - s_p0 is exact in float32 (tests/test_loss_kernel_host.py).  Each special exponent is a positive in
    the even rows and a negative in the odd ones, or the other way round."""
    B, tau = CLAMP_B, CLAMP_TAU
    S = np.zeros((B, B), dtype=np.float64)
    pos = uniform(77, B, B) < -0.4
    neg = (uniform(78, B, B) < 0.2) & ~pos
    idx = np.zeros((B, 2), dtype=np.int64)
    moderate = np.round(uniform(79, B, B) * 8.0 * 2.0 ** 10) / 2.0 ** 10
    special_cols = {}
    for q in range(B):
        p0, p1 = (q + 1) % B, (q + 2) % B
        base = CLAMP_BASES[q % 3]
        e = moderate[q].copy()
        others = [z for z in range(B) if z not in (p0, p1)]
        cols = [others[(11 * q + 6 * k) % len(others)] for k in range(10)]
        assert len(set(cols)) == 10
        for k, (z, ex) in enumerate(zip(cols, clamp_exponents())):
            e[z] = ex
            pos[q, z], neg[q, z] = (k + q) % 2 == 0, (k + q) % 2 == 1
        e[p0], e[p1] = 0.0, 3.0
        S[q] = base - e * tau
        pos[q, [p0, p1]], neg[q, [p0, p1]] = True, False
        idx[q] = (p0, p1)
        special_cols[q] = cols
    assert (S.astype(np.float32).astype(np.float64) == S).all()
    return _case(torch.from_numpy(S.astype(np.float32)), torch.from_numpy(pos), torch.from_numpy(neg), torch.from_numpy(idx),
                 tau), special_cols


TIE_ROW, TIE_COUNT = 5, 100


def smoothap_ties(tau=TAU):
    """B = 257, P = 4: in row TIE_ROW, 100 elements (30 positives, 50 negatives, 20 neither) equal the best positive to the bit."""
    B, P = FAMILY_B, FAMILY_P
    S, pos, neg = _random_parts(B, 5151)
    q = TIE_ROW
    best = max((z for z in range(B) if pos[q, z]), key=lambda z: S[q, z])
    cols = [z for z in range(B) if z not in (q, best)][3::2][:TIE_COUNT]
    S[q, cols] = S[q, best]
    pos[q, cols], neg[q, cols] = False, False
    pos[q, cols[:30]] = True
    neg[q, cols[30:80]] = True
    S, pos, neg = torch.from_numpy(S), torch.from_numpy(pos), torch.from_numpy(neg)
    return _case(S, pos, neg, top_positives(S, pos, P), tau), cols


def sample_rows(B, n=64, seed=99):
    """n distinct hash-chosen rows of a batch of B, the first and the last among them, sorted."""
    picked = [0, B - 1]
    for r in ((uniform(seed + B, 8 * n) + 1.0) * 0.5 * B).astype(np.int64) % B:
        if len(picked) < n and int(r) not in picked:
            picked.append(int(r))
    return torch.tensor(sorted(picked), dtype=torch.int64)


def smoothap_lds(B, P, device='cpu', rows=None, tau=TAU):
    """A batch too large to draw element by element on the host: S[q, z] = w[q + z], pos[q, z] = hp[3 q + z] < -0.8,
    neg[q, z] = hn[2 q + z] < 1/3 and not pos, the diagonal neither, from three hash vectors of 2 B, 4 B and 3 B values; idx
    the true top-P positives.  Any subset `rows` of the batch can be built alone (the float64 side of the largest sizes)."""
    w = torch.from_numpy(uniform(B, 2 * B).astype(np.float32)).to(device)
    hp = torch.from_numpy(uniform(B + 1, 4 * B)).to(device)
    hn = torch.from_numpy(uniform(B + 2, 3 * B)).to(device)
    S = w.as_strided((B, B), (1, 1))
    pos = hp.as_strided((B, B), (3, 1)) < -0.8
    neg = hn.as_strided((B, B), (2, 1)) < 1.0 / 3.0
    q = torch.arange(B, device=device) if rows is None else rows.to(device)
    S, pos, neg = S[q].contiguous(), pos[q].clone(), neg[q].clone()
    neg &= ~pos
    at = torch.arange(q.numel(), device=device)
    pos[at, q] = False
    neg[at, q] = False
    return _case(S, pos, neg, top_positives(S, pos, P), tau)


# ================================================================================================ KD: reference
KdRef = collections.namedtuple('KdRef', 'kl grad kl_scale grad_scale sum_scale')


def kd_ref(y, t, T, dtype=torch.float64):
    """Per row KL(softmax(t / T) || softmax(y / T)) and its derivative (p - q) / T with respect to y (loss.py:138-147 without
    the batch mean and the weight).  The scales are the magnitudes of the terms each quantity is made of, the two
    distributions counted separately, as an fp32 implementation has to form them:
      grad_scale = max_j (p_j + q_j) / T        for an entry (p_j - q_j) / T,
      kl_scale   = sum_j q_j (|log q_j| + |log p_j|)    for kl = sum_j q_j log q_j - sum_j q_j log p_j,
      sum_scale  = sum_j (p_j + q_j) / T = 2 / T         for the sum of a gradient row, (sum_j p_j - sum_j q_j) / T."""
    T = f32(T)
    lp = torch.log_softmax(y.to(dtype) / T, dim=1)
    lq = torch.log_softmax(t.to(dtype) / T, dim=1)
    p, q = lp.exp(), lq.exp()
    return KdRef((q * (lq - lp)).sum(1), (p - q) / T, (q * (lq.abs() + lp.abs())).sum(1), ((p + q) / T).amax(1),
                 ((p + q) / T).sum(1))


def kd_ref64(y, t, T):
    r = kd_ref(y, t, T, torch.float64)
    return r.kl, r.grad


def kd_ref32(y, t, T):
    r = kd_ref(y, t, T, torch.float32)
    return r.kl, r.grad


# ================================================================================================ KD: cases
KD_DIMS = tuple(range(64, 1025, 64))                          # K = D / 64 = 1 .. 16: every instantiation
KD_BATCHES = (1, 3, 4, 5, 257)                                # 4 rows per workgroup: a part-filled one, a full one, one more
KD_TEMPERATURES = (0.5, 3.0, 20.0)
KD_T = 3.0                                                    # loss.py:139
KD_CLOSE = tuple((noise, d) for noise in (1e-3, 1e-6) for d in (64, 256, 1024))
KD_UNDERFLOW = (64, 200.0, 0.25)                              # (D, scale, T): (t - max t) / T reaches below -104


def _t(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in arrays)


def kd_width(batch, dim, scale=1.0):
    return _t(*syn.kd_case(100 * dim + batch, batch, dim, scale))


def kd_close(noise, dim, batch=5):
    """teacher = student + noise * u, u uniform in (-1, 1) per entry: what the kernel's expm1 / log1p form is for"""
    y, _ = syn.kd_case(300 + dim, batch, dim)
    return _t(y, y.astype(np.float64) + noise * uniform(301 + dim, batch, dim))


def kd_mixed(dim, batch=6):
    """`kd_close(1e-3)` except three entries per row, where the teacher differs by +5T, -5T, -5T (even rows) or by -5T three
    times (odd rows).  After the kernel's max-subtraction the +5T entry is the teacher's maximum: in an even row it alone
    has |delta| < 1, in an odd row all but the three have."""
    y, t = kd_close(1e-3, dim, batch)
    t = t.clone()
    for r in range(batch):
        cols = [(17 * r + 3) % dim, (29 * r + 40) % dim, (r + 57) % dim]
        assert len(set(cols)) == 3
        signs = (1.0, -1.0, -1.0) if r % 2 == 0 else (-1.0, -1.0, -1.0)
        for c, s in zip(cols, signs):
            t[r, c] = y[r, c] + s * 5.0 * KD_T
    return y, t


def kd_peaked(dim, batch=5):
    """(peaked, flat): rows of 0.01 u with one entry at 10 T, and rows of 0.01 u.  Student peaked and teacher flat gives
    Zp / Zq - 1 = (1 + (D - 1) e^-10) / D - 1 <= -0.5, the kernel's logf(1 + x) branch; the converse gives x of about D."""
    peaked = 0.01 * uniform(400 + dim, batch, dim)
    flat = 0.01 * uniform(401 + dim, batch, dim)
    for r in range(batch):
        peaked[r, (13 * r + 5) % dim] = 10.0 * KD_T
    return _t(peaked, flat)


KD_SHIFTS = (1e4, -3000.0)


def kd_shifted(dim=256, batch=5):
    """((y, t), (y + 1e4, t - 3000)) with y, t multiples of 2^-8 (scale 20), so both shifts are exact in float32."""
    y, t = syn.kd_case(500 + dim, batch, dim, 20.0)
    y, t = np.round(y.astype(np.float64) * 256.0) / 256.0, np.round(t.astype(np.float64) * 256.0) / 256.0
    return _t(y, t), _t(y + KD_SHIFTS[0], t + KD_SHIFTS[1])


# ================================================================================================ bars
def row_bars(e32, scale, close=False):
    """2 E32 + 2^-22 scale per row; `close`: E32 itself (the close-rows cases of the distillation kernel)."""
    return e32 if close else 2.0 * e32 + FLOOR * scale


def bar_use(err, bar):
    """Largest err / bar over the rows; a row whose bar is 0 must have no error at all."""
    zero = bar == 0
    assert bool((err[zero] == 0).all()), 'a row whose bar is exactly 0 carries an error'
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bar[~zero]).max())
