"""float64 reference of the row decompressor (csrc/decompress_rows_impl.h) that yields, for every output element, the SET of fp16
values a correct kernel may produce, the cases tests/test_gpu_decompress.py runs on the GPU and tests/test_decomp_ref_cpu.py proves
on the CPU, and a mirror of the entry point's dispatch rules.  numpy only.

    out = fp16( fp16(dequant(code)) + sum_c Q[t,c] P[d,c] ),   outlier positions: out = fp16( value + sum_c ... )

What is bit-determined is modelled bit-exactly (`base_values`):
  mode 0   dequant_one<0> (common.h): hround(hround(q * scale) + mn).  q <= 255 and an fp16 scale: the fp32 product is exact, so the
           inner hround is ONE rounding of the float64 product; the fp32 sum of two fp16 values followed by hround equals the direct
           fp16 rounding of their float64 sum (24 >= 2 * 11 + 2).
  mode 1   dequant_one<1>: __fmul_rn, __fadd_rn in fp32, then the cast to fp16 (pack8 / f2h2_bits in dense_row) -- np.float32
           arithmetic is the same correctly rounded arithmetic.
  outliers fill_table / refill: an entry of oidx below the row length replaces the dequantized value by oval's bits (dense_row's sel);
           an index at or beyond the row length (the 0xFFFF padding of a head shard's list) is an unused slot.
  rank 0   nothing is added (compute_row: `if (r > 0)`): the set is the base value alone, the comparison is bit for bit.

What is not bit-determined is the order of the fp32 additions of the low-rank term.  The products Q[t,c] P[d,c] of two fp16 values
are exact in fp32 (22 bits) and in float64, so exact = base + sum_c Q P in float64 carries only float64's own error
(r * 2^-53 * sum |Q P|), and the three implementations differ from it by their fp32 roundings alone:
  compute_row, RV > 0   `acc = f[j]` then RV / 2 v_dot2_f32_f16 onto it: at most 2 roundings per instruction = r roundings
  compute_row, RV == 0  `acc = fmaf(fv[c], g, acc)` r times from 0 (the first is exact) and `f[j] += acc`: r roundings
  compute4 (rank 4 / 8) accumulators start from the dequantized values, RV / 4 v_mfma_f32_4x4x4f16 of 4 products each: at most 4
                        roundings per instruction = r roundings
Every partial sum is at most (|base| + sum |Q P|) (1 + 2^-24)^r in magnitude, so i roundings cost at most i * 2^-24 * (|base| +
sum |Q P|) (1 + 2^-24)^i, and with i <= r <= 16 that is below
  e = (r + 1) * 2^-24 * (|base| + sum_c |Q P|)
in any order of the additions.  The admissible values are the fp16 roundings of [exact - e, exact + e] (rounding is monotone: the
run between the roundings of the ends).  +0 and -0 count as one value (dense_ref.key).

Subnormal fp16 factor entries: whether v_dot2_f32_f16 / v_mfma_f32_4x4x4f16 honour them is a property of the hardware mode, so
`decomp_sets(flush=True)` gives the sets with such operands read as zero; the GPU test asks for one of the two, whole.

The cases (`gpu_cases`) are synthetic payloads built from a seed: positions and values of the outliers are chosen (row seams, word
halves, the lane 31 / 32 store seam, one lane's 16 columns, the same column in neighbouring rows and across a 128-row block, empty
and padded lists, +-0, +-65504, the smallest subnormal).  So that a set holds at most two values, codes and outlier values are
conditioned on the REFERENCE's own quantities, never on a kernel's output: an element whose |exact| would fall below
(r + 1) * 2^-11 * (|base| + sum |Q P|) = 2^13 e (the interval would then span more than one rounding boundary) takes the next code /
an ordinary value of the low-rank term's sign."""
import functools
import zlib

import numpy as np

from dense_ref import SENTINEL, Sets, U, assert_admissible, assert_bits, f16, mismatches, rnd   # noqa: F401 (re-exported)

HD = 128                  # head dimension of every case
PAD = 0xFFFF              # unused outlier slot
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------- payload layouts
def unpack(code, bits):
    """int32 words [..., W] -> codes uint8 [..., W * 32 / bits], least significant first."""
    w = np.ascontiguousarray(code).view(np.uint32)
    sh = (np.arange(32 // bits, dtype=np.uint32) * bits)
    q = (w[..., None] >> sh) & np.uint32((1 << bits) - 1)
    return q.reshape(w.shape[:-1] + (-1,)).astype(np.uint8)


def pack(q, bits):
    fpi = 32 // bits
    v = q.astype(np.uint32).reshape(q.shape[:-1] + (q.shape[-1] // fpi, fpi))
    sh = (np.arange(fpi, dtype=np.uint32) * bits)
    return np.bitwise_or.reduce(v << sh, axis=-1).astype(np.uint32).view(np.int32)


def out_shape(kind, B, H, T, D):
    """The decompressor's output: V [B, H, T, D], K^T [B, H, D, T]."""
    return (B, H, T, D) if kind == "v" else (B, H, D, T)


def row_geometry(kind, B, H, T, D):
    """(n_rows, rows_inner, row length) of gear_decompress_rows as compress.decompress calls it."""
    return (B * T, T, H * D) if kind == "v" else (B * H * D, D, T)


def to_rows(kind, x):
    """Output layout -> the kernel's row matrix [n_rows, len]: V row (b, t) = the heads' channels side by side, K^T row (bh, d)."""
    if kind == "v":
        B, H, T, D = x.shape
        return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B * T, H * D)
    return np.ascontiguousarray(x).reshape(-1, x.shape[-1])


def from_rows(kind, rows, B, H, T, D):
    if kind == "v":
        return np.ascontiguousarray(rows.reshape(B, T, H, D).transpose(0, 2, 1, 3))
    return np.ascontiguousarray(rows.reshape(B, H, D, T))


def outlier_index(kind, oidx, B, H, T, D):
    """The list slots that hold an outlier -> (index tuple into the output layout, (row, slot) of the entries)."""
    n_rows, _, length = row_geometry(kind, B, H, T, D)
    oi = np.ascontiguousarray(oidx).view(np.uint16).astype(np.int64).reshape(n_rows, -1)
    rows, slots = np.nonzero(oi < length)
    j = oi[rows, slots]
    if kind == "v":
        return (rows // T, j // D, rows % T, j % D), (rows, slots)
    return (rows // (H * D), rows // D % H, rows % D, j), (rows, slots)


# ------------------------------------------------------------------------------------------------------------------ reference
def dequant(q, scale, mn, group, mode):
    """fp16 value of every code (groups along the last dimension in both layouts)."""
    s, m = np.repeat(scale, group, -1), np.repeat(mn, group, -1)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == 0:
            return f16(rnd(q.astype(F64) * s.astype(np.float16).astype(F64)) + m.astype(np.float16).astype(F64))
        return (q.astype(F32) * s.astype(F32) + m.astype(F32)).astype(np.float16)


def base_values(code, scale, mn, oidx, oval, kind, bits, group, mode, B, H, T, D, k):
    """fp16(dequant(code)) with the outliers restored, in the output layout: one exact fp16 value per element."""
    base = dequant(unpack(code, bits), scale, mn, group, mode).reshape(out_shape(kind, B, H, T, D))
    if k > 0:
        idx, (rows, slots) = outlier_index(kind, oidx, B, H, T, D)
        base[idx] = np.ascontiguousarray(oval).view(np.float16).reshape(-1, 2 * k)[rows, slots]
    return base


def _flushed(a):
    a = np.asarray(a, np.float16).astype(F64)
    return np.where(np.abs(a) < 2.0 ** -14, 0.0, a)


def lowrank_terms(P, Q, kind, flush=False):
    """(sum_c Q[t,c] P[d,c], sum_c |Q P|) in float64, in the output layout.  V: bh = the element's head, t = the row's token, d =
    the channel; K^T: bh = the row's head, d = the row's channel, t = the element."""
    conv = _flushed if flush else (lambda a: np.asarray(a, np.float16).astype(F64))
    p, q = conv(P), conv(Q)
    a, b = (q, p) if kind == "v" else (p, q)
    return np.matmul(a, b.swapaxes(-1, -2)), np.matmul(np.abs(a), np.abs(b).swapaxes(-1, -2))


def bound(r, base, S):
    """e of the module docstring (plus float64's own error of the sum)."""
    return (r + 1) * U * (np.abs(base) + S) + r * 2.0 ** -53 * S


def decomp_sets(code, scale, mn, P, Q, oidx, oval, kind, bits, group, mode, B, H, T, D, r, k, flush=False, lr_at_outliers=True):
    """Sets of the admissible fp16 values of every output element.  lr_at_outliers=False is a WRONG decompressor (the low-rank term
    missing at outlier positions) for the negative controls."""
    base = base_values(code, scale, mn, oidx, oval, kind, bits, group, mode, B, H, T, D, k)
    if r == 0:
        return Sets.exact(base)
    lr, S = lowrank_terms(P, Q, kind, flush)
    if not lr_at_outliers and k > 0:
        idx, _ = outlier_index(kind, oidx, B, H, T, D)
        lr[idx], S[idx] = 0.0, 0.0
    b = base.astype(F64)
    e = bound(r, b, S)
    return Sets.interval(b + lr, b + lr - e, b + lr + e)


def case_sets(c, **kw):
    return decomp_sets(c["code"], c["scale"], c["mn"], c["P"], c["Q"], c["oidx"], c["oval"], c["kind"], c["bits"], c["group"],
                       c["mode"], c["B"], c["H"], c["T"], HD, c["r"], c["k"], **kw)


# ------------------------------------------------------------------------------------------- the entry point's dispatch rules
def dispatch(kind, bits, B, H, T, r, k, rpb_opt=0, general=0, D=HD):
    """gear_decompress_rows' host code and the kernel's `fast` condition, restated: which flavour a call selects."""
    n_rows, rows_inner, length = row_geometry(kind, B, H, T, D)
    lpr = length // 16
    rpb = 16
    while rpb > 1 and rows_inner % rpb:
        rpb >>= 1
    rpar = 1
    if lpr < 64 and 64 % lpr == 0:
        rp = 64 // lpr
        rb = 16 * rp
        while rb > rp and rows_inner % rb:
            rb >>= 1
        if rows_inner % rb == 0:
            rpar, rpb = rp, rb
    if r in (4, 8) and rpar == 1 and rpb == 16 and bits <= 4 and length % 1024 == 0 and length <= 8192 and not general:
        for c in (128, 64, 32):
            if rows_inner % c == 0 and n_rows % c == 0 and (c == rpb_opt if rpb_opt > 0 else (rpb_opt == 0 and n_rows // c >= 1024)):
                rpb = c
                break
    trows = min(rpb, 4)
    while trows > 1 and (rpb % trows or trows * ((length // 32 + 1) * 4 + length * 2) > 72 * 1024):
        trows >>= 1
    trows = max(trows, rpar)
    threads = (lpr + 63) // 64 * 64
    tb = 256 if threads <= 256 else 512 if threads <= 512 else 1024
    nblocks = (n_rows + rpb - 1) // rpb
    rv = r if r in (4, 8, 16) else 0
    pf_ok = trows * 2 * k <= 2 * threads
    # (rpb divides rows_inner, which divides n_rows: every block is full)
    fast = (bits <= 4 and not general and (rv > 0 or r == 0) and
            (rpb == 16 * rpar or (rv in (4, 8) and tb < 1024 and rpar == 1 and rpb % 8 == 0 and rpb > 16)) and
            (tb == 256 if rpar > 1 else trows == 4) and (k == 0 or pf_ok))
    full_waves = threads // 64 if rpar > 1 else length // 1024
    waves = threads // 64
    if not fast or full_waves == 0:
        loop = "general"
    elif rpar > 1:
        loop = "straight x%d" % rpar
    elif rv in (4, 8) and tb < 1024:
        loop = "mfma16" if rpb == 16 else "mfma rolled %d" % rpb
    else:
        loop = "straight"
    if loop != "general" and full_waves < waves:
        loop += " + general (last wave)"
    arith = "none" if r == 0 else "fmaf" if rv == 0 else "mfma" if loop.startswith("mfma") else "fdot2"
    if loop.startswith("mfma") and full_waves < waves:
        arith = "mfma + fdot2"
    swap = full_waves > 0 and (loop != "general" or rpar == 1)       # (the general loop exchanges store halves on whole waves of one row)
    return dict(rpb=rpb, rpar=rpar, trows=trows, threads=threads, tb=tb, nblocks=nblocks, rv=rv, pf_ok=pf_ok, loop=loop, arith=arith,
                shmem=trows * length * 2 if k else 0, xcd=bool(kind == "k" and r > 0 and nblocks % 8 == 0), swap=bool(swap),
                length=length, n_rows=n_rows)


def case_dispatch(c):
    return dispatch(c["kind"], c["bits"], c["B"], c["H"], c["T"], c["r"], c["k"], c["rpb"], c["general"])


def xcd_order(nblocks):
    """Launch index -> block, as the kernel's XCD-contiguous remap computes it (grid a multiple of 8)."""
    i = np.arange(nblocks)
    return (i & 7) * (nblocks >> 3) + (i >> 3)


# ------------------------------------------------------------------------------------------------------------- case makers
def _margin(r):
    return (r + 1) * 2.0 ** -11


def _outlier_lists(rng, n_rows, length, k):
    """uint16 [n_rows, 2k]: both sides sorted, all 2k distinct in a row; the chosen positions of the module docstring."""
    n = 2 * k
    oi = np.argpartition(rng.random((n_rows, length)), n - 1, axis=1)[:, :n] if n < length else np.tile(np.arange(length), (n_rows, 1))

    def take(cands, row):
        seen = []
        for c in list(cands) + [int(v) for v in oi[row]]:
            if 0 <= c < length and c not in seen:
                seen.append(c)
        if len(seen) < n:
            seen += [c for c in range(length) if c not in seen]
        return seen[:n]

    lane = min(33, length // 16 - 1)
    patterns = {
        0: [0, length - 1, 1, 15, 16, 17],                                  # row ends, both halves of a word, a lane's last / next first
        1: [15, 16, 14, 17, 0, length - 1],
        2: [511, 512, 510, 513, 509, 514] if length > 512 else [30, 31, 32, 33],      # the lane 31 / 32 store-exchange seam
        7: [16 * lane + v for v in (0, 15, 1, 14, 7, 8, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13)] if n <= 16 else [],   # one lane's columns
        8: [6, 7, 22, 23, 38, 39],                                          # pairs inside one 32-bit word
    }
    for row, cands in patterns.items():
        if row < n_rows and cands:
            oi[row] = take(cands, row)
    oi = np.sort(oi, 1)
    oi = np.concatenate([oi[:, 0::2], oi[:, 1::2]], 1).astype(np.int64)     # small side | large side, each sorted
    if n_rows > 5:
        oi[5] = PAD                                                         # a row with no real outlier between full rows
    if n_rows > 6:
        oi[6, k - 1] = PAD                                                  # a partly padded list (a head shard's)
    for a in (3, 15, 127):                                                  # the same columns in rows 3 | 4, 15 | 16, 127 | 128
        if a + 1 < n_rows:
            oi[a + 1] = oi[a]
    return oi.astype(np.uint16)


def _outlier_values(rng, oi, lr_at, S_at, r, cancel):
    """fp16 values for the list entries (lr_at, S_at: the low-rank term and sum |Q P| at each entry's position; 0 for rank 0)."""
    n_rows, n = oi.shape
    ordinary = rng.standard_normal(oi.shape) * 3.0
    ordinary = np.where(np.abs(ordinary) < 0.05, 0.05, ordinary)
    sgn_lr = np.where(lr_at < 0, -1.0, 1.0)
    if cancel:
        val = rnd(-lr_at + rng.choice([-1.0, 1.0], oi.shape) * S_at / 40)
    else:
        sel = (np.arange(n_rows)[:, None] * 5 + np.arange(n)[None, :] * 3) % 10
        # (+-65504 against the low-rank term's sign, so that the exact value stays finite; rank 0: both signs)
        big = -sgn_lr if r > 0 else np.where(np.arange(n_rows)[:, None] % 4 < 2, 1.0, -1.0) * np.ones(oi.shape)
        special = np.select([sel == 0, sel == 1, sel == 2, sel == 3, sel == 4],
                            [0.0, -0.0, big * 65504.0, 2.0 ** -24, -2.0 ** -24], ordinary)
        val = rnd(special)
        if r > 0:
            bad = np.abs(val + lr_at) < 2 * _margin(r) * (np.abs(val) + S_at)
            val = np.where(bad, rnd(sgn_lr * (np.abs(ordinary) + S_at / 8)), val)
    val = np.where(oi == PAD, 0.0, val)
    return f16(val)


def make_case(name, kind, B, H, T, bits=2, group=64, mode=1, r=0, k=0, fscale=0.3, rpb=0, general=0, flavour="", guard=False):
    """One synthetic payload, seeded by its name.  Scales and zero points give KV-like values in about [-4, 4] (mode 0: fp16, mode 1:
    float32 with full mantissas; 2 fscale^2 times that next to factors of scale 4, whose term is of that size); factors Gaussian * fscale without subnormal entries -- flavour "subnormal": Q all subnormal
    (m * 2^-24) against P of +-2^13 .. 2^14, flavour "cancel": every outlier value within sum |Q P| / 32 of minus the low-rank term."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    shape = out_shape(kind, B, H, T, HD)
    n_rows, _, length = row_geometry(kind, B, H, T, HD)
    levels = (1 << bits) - 1
    gshape = shape[:-1] + (shape[-1] // group,)
    span = rng.uniform(2.0, 6.0, gshape) * (2 * fscale * fscale if (r and fscale > 1) else 1.0)     # (values of the factors' size)
    mn = -span * rng.uniform(0.35, 0.65, gshape)
    sdt = np.float16 if mode == 0 else F32
    scale, mn = (span / levels).astype(sdt), mn.astype(sdt)
    P = Q = None
    lr = S = np.zeros(shape)
    if r > 0:
        if flavour == "subnormal":
            Q = (rng.integers(1, 1024, (B, H, T, r)).astype(np.uint16) | (rng.integers(0, 2, (B, H, T, r)).astype(np.uint16) << 15)).view(np.float16)
            P = f16(2.0 ** 13 * (1 + rng.random((B, H, HD, r))) * rng.choice([-1.0, 1.0], (B, H, HD, r)))
        else:
            def factor(*s):
                a = rnd(rng.standard_normal(s) * fscale)
                return f16(np.where(np.abs(a) < 2.0 ** -14, 2.0 ** -10, a))
            P, Q = factor(B, H, HD, r), factor(B, H, T, r)
        lr, S = lowrank_terms(P, Q, kind)
    oidx = oval = None
    at = None
    if k > 0:
        oi = _outlier_lists(rng, n_rows, length, k)
        at, (rows, slots) = outlier_index(kind, oi, B, H, T, HD)
        lr_at, S_at = np.zeros(oi.shape), np.zeros(oi.shape)
        lr_at[rows, slots], S_at[rows, slots] = lr[at], S[at]
        oidx, oval = oi, _outlier_values(rng, oi, lr_at, S_at, r, flavour == "cancel")
    q = rng.integers(0, levels + 1, shape).astype(np.uint8)
    if r > 0:       # (see the module docstring: no element's interval may span two rounding boundaries)
        b = dequant(q, scale, mn, group, mode).astype(F64)
        bad = np.abs(b + lr) < 2 * _margin(r) * (np.abs(b) + S)
        q[bad] = np.where(lr[bad] < 0, 0, levels)      # the group's lowest (negative) / highest (positive) value, of the term's sign
    c = dict(name=name, kind=kind, B=B, H=H, T=T, bits=bits, group=group, mode=mode, r=r, k=k, rpb=rpb, general=general, flavour=flavour,
             guard=guard, code=pack(q, bits), scale=scale, mn=mn, P=P, Q=Q, oidx=oidx, oval=oval)
    _check_case(c, lr, S)
    return c


def _check_case(c, lr, S):
    """The conditions on the inputs: a finite exact value everywhere, no interval wider than one rounding boundary, and the
    near-cancelling flavour within its bounds."""
    base = base_values(c["code"], c["scale"], c["mn"], c["oidx"], c["oval"], c["kind"], c["bits"], c["group"], c["mode"], c["B"], c["H"],
                       c["T"], HD, c["k"]).astype(F64)
    exact = base + lr
    assert np.isfinite(base).all() and (np.abs(exact) <= 65504).all(), c["name"]
    if c["r"] > 0:
        assert (np.abs(exact) >= _margin(c["r"]) * (np.abs(base) + S)).all(), c["name"]
    if c["flavour"] == "cancel":
        at, _ = outlier_index(c["kind"], c["oidx"], c["B"], c["H"], c["T"], HD)
        assert len(at[0]) and (np.abs(exact[at]) <= S[at] / 32).all(), c["name"]


# -- the shapes of the issue's tables: (H, T) for V rows of H * 128 elements, (BH, T) for K^T rows of T elements (128 rows per head)
V_SHAPES = [(1, 128), (2, 64), (4, 32), (1, 40), (2, 40), (4, 40), (1, 17), (3, 16), (8, 16), (10, 16), (32, 16), (64, 16), (128, 16)]
K_SHAPES = [(2, 16), (2, 64), (1, 640), (2, 1024), (1, 1280), (1, 2048), (1, 4096), (1, 8192), (2, 16384)]
GUARDED_V = {(10, 16), (64, 16)}
RUNTIME_RANKS = (1, 2, 5, 12)
TRIPLES = [(b, m, k) for k in (0, 1, 3) for m in (1, 0) for b in (2, 4)]      # (bits, mode, k): all twelve


def _spec(kind, a, t, **kw):
    d = dict(kind=kind, B=kw.pop("B", 1), H=a, T=t, bits=2, group=64, mode=1, r=0, k=0, fscale=0.3, rpb=0, general=0, flavour="", guard=False)
    d.update(kw)
    return d


def _name(s):
    n = "%s-H%d-T%d-b%d-m%d-r%d-k%d" % (s["kind"], s["H"], s["T"], s["bits"], s["mode"], s["r"], s["k"])
    if s["B"] != 1:
        n += "-B%d" % s["B"]
    if s["group"] != 64:
        n += "-g%d" % s["group"]
    if s["fscale"] != 0.3 and s["r"]:
        n += "-f%g" % s["fscale"]
    if s["rpb"] or s["general"]:
        n += "-rpb%d-gen%d" % (s["rpb"], s["general"])
    if s["flavour"]:
        n += "-" + s["flavour"]
    return n


def case_specs():
    """Every GPU case as make_case's keyword arguments (no arrays yet), in a fixed order: {name: spec}, and the names of the two
    guarded cases the negative controls use."""
    specs = {}

    def add(kind, a, t, **kw):
        s = _spec(kind, a, t, **kw)
        specs.setdefault(_name(s), s)
        return _name(s)
    for kind, shapes in (("v", V_SHAPES), ("k", K_SHAPES)):
        for si, (a, t) in enumerate(shapes):
            ranks = [0, (4, 8)[si % 2], 16, RUNTIME_RANKS[si % 4]]
            big = (a * HD if kind == "v" else t) * (t if kind == "v" else a * HD) >= 1 << 20
            per_rank = 1 if big else 3          # (a reference of a million elements and more: one triple per rank)
            for ri, r in enumerate(ranks):
                for j in range(per_rank):
                    bits, mode, k = TRIPLES[(3 * ri + j + 5 * si) % 12]
                    add(kind, a, t, bits=bits, mode=mode, r=r, k=k, fscale=(0.3, 4.0)[(ri + j + si) % 2],
                        group=16 if (kind == "k" and t < 64) else 64,        # (a K^T row of 16 tokens holds no group of 64)
                        guard=kind == "v" and (a, t) in GUARDED_V)
    # 8-bit codes at two shapes per kind; groups of 32 and 128 once each
    for kind, a, t in (("v", 8, 16), ("v", 1, 128), ("k", 2, 1024), ("k", 2, 64)):
        add(kind, a, t, bits=8, mode=1, r=8, k=3)
        add(kind, a, t, bits=8, mode=0, r=0, k=1)
        add(kind, a, t, bits=8, mode=1, r=5, k=0, fscale=4.0)
    add("v", 8, 16, group=32, r=8, k=3)
    add("v", 8, 16, group=128, r=16, k=3, mode=0, bits=4)
    add("k", 2, 1024, group=128, r=4, k=3)
    add("k", 2, 1024, group=32, r=2, k=1, mode=0, bits=4)
    # rows per workgroup behind one factor-block load (rank 4 / 8, rows of a multiple of 1024 elements), and the general loop
    for kind, a, t, B in (("v", 8, 128, 2), ("k", 2, 1024, 1)):
        for rpb in (-1, 32, 64, 128):
            for general in (0, 1):
                i = len(specs)
                add(kind, a, t, B=B, r=(4, 8)[i % 2], bits=(2, 4)[(i // 2) % 2], k=(3, 0, 1)[i % 3], mode=1 - (i // 3) % 2,
                    fscale=(0.3, 4.0)[i % 2], rpb=rpb, general=general)
    for rpb in (32, 64, 128):
        add("k", 1, 2048, r=8, k=3, rpb=rpb)
        add("k", 1, 4096, r=4, k=1, bits=4, rpb=rpb, fscale=4.0)
        add("v", 32, 128 if rpb == 128 else 64, r=8, k=3, rpb=rpb)
    # the XCD-contiguous block order: off with 3 blocks, on with 8
    for bh in (3, 8):
        for r, k, bits in ((8, 3, 2), (4, 0, 4), (8, 1, 2)):
            add("k", bh, 1024, r=r, k=k, bits=bits, rpb=128, guard=True, fscale=(0.3, 4.0)[k % 2])
    # both sides of the prefetch limit trows * 2k <= 2 * threads
    for k in (16, 17):
        for r in (0, 8, 16):
            add("k", 2, 1024, r=r, k=k)
    for k in (64, 65):
        for r in (0, 8, 5):
            add("v", 32, 16, r=r, k=k, bits=(2, 4)[k % 2])
    # the near-cancelling outlier values and the subnormal factor entries
    add("k", 2, 1024, r=16, k=3, fscale=4.0, flavour="cancel")
    add("v", 8, 16, r=8, k=3, fscale=4.0, flavour="cancel")
    add("v", 4, 40, r=5, k=3, flavour="cancel")
    controls = [add("v", 10, 16, r=8, k=3, guard=True), add("k", 8, 1024, r=8, k=3, rpb=128, guard=True, fscale=4.0)]
    for s in subnormal_specs():
        specs.setdefault(_name(s), s)
    return specs, controls


def subnormal_specs():
    """One case per arithmetic: v_dot2_f32_f16 (straight-line, general loop, short rows), fmaf (runtime rank), matrix cores (16 rows
    and rolled)."""
    return [_spec("k", 2, 1024, r=16, k=3, flavour="subnormal"), _spec("k", 2, 1024, r=8, k=3, general=1, flavour="subnormal"),
            _spec("v", 2, 64, r=8, k=1, flavour="subnormal"), _spec("v", 8, 16, r=5, k=3, flavour="subnormal"),
            _spec("k", 2, 1024, r=8, k=3, flavour="subnormal"), _spec("k", 2, 1024, r=4, k=0, rpb=64, flavour="subnormal")]


_SPECS, NEGATIVE_CONTROLS = case_specs()
CASE_NAMES = list(_SPECS)
SUBNORMAL_NAMES = [_name(s) for s in subnormal_specs()]


@functools.lru_cache(maxsize=4)
def get_case(name):
    """The case and its sets, built once and shared (treat both as read-only)."""
    c = make_case(name, **_SPECS[name])
    return c, case_sets(c)


# ------------------------------------------------------------------------------------------------ wrong decompressors (inputs)
def shifted_table(c, trows):
    """The case with its outlier lists as a decompressor would see them whose LDS table is one fill late: in every block of 2 * trows
    rows the second fill's rows read the first fill's lists."""
    oi, ov = c["oidx"].copy(), c["oval"].copy()
    rows = np.arange(oi.shape[0])
    late = rows[(rows // trows) % 2 == 1]
    oi[late], ov[late] = c["oidx"][late - trows], c["oval"][late - trows]
    return dict(c, oidx=oi, oval=ov)


def next_group_scale(c):
    return dict(c, scale=np.roll(c["scale"], -1, -1))
