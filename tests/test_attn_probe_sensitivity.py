"""The probe bounds sit between rounding noise and one-token bugs (CPU only, no GPU): on synthetic caches with realistic outlier,
segment, window and chunk layouts, the fp16-shaped reference (tests/attn_probe.py) stays within a third of ROW_BOUND / LSE_BOUND on
every probe family, and every mutation M1 - M9 of the reference that applies to a shape moves the probes' results past 5x a
bound."""
import numpy as np
import pytest

import attn_probe as AP

D = AP.D


def synthetic_parts(seed, B, Hkv, T, W, n, bits, rk, rv, seg0, seglen, kk0, kkb, kv, group=64):
    """parts of a cache as the compress kernels leave it: group-wise quantized Gaussian backbone, per-segment rank-r factors,
    K outlier lists (kk0 per side over the prompt segment, kkb per side and decode-time block, at the list positions the cache
    uses), V outlier lists (kv per side and token row, columns over all heads), fp16 window and chunk rows."""
    rng = np.random.default_rng(seed)
    levels = (1 << bits) - 1

    def quant(x, axis):         # asymmetric min / max quantization in groups along `axis` (fp16 scale and minimum)
        x = np.moveaxis(x, axis, -1)
        g = x.reshape(x.shape[:-1] + (-1, group))
        mn = AP.f16(g.min(-1, keepdims=True))
        sc = AP.f16((g.max(-1, keepdims=True) - mn) / levels)
        code = np.clip(np.round((g - mn) / np.maximum(sc, 1e-8)), 0, levels)
        return np.moveaxis((code * sc + mn).reshape(x.shape), -1, axis)

    Kd = quant(rng.standard_normal((B, Hkv, T, D)), 2) if T else np.zeros((B, Hkv, 0, D))
    Vd = quant(rng.standard_normal((B, Hkv, T, D)), 3) if T else np.zeros((B, Hkv, 0, D))
    seg = np.zeros(T, np.int64)
    if seglen:
        seg[seg0:] = 1 + (np.arange(seg0, T) - seg0) // seglen
    nseg = int(seg.max()) + 1 if T else 1
    fac = lambda *s: AP.f16(0.25 * rng.standard_normal(s))
    parts = dict(Kd=Kd, Vd=Vd, seg=seg, seg0=seg0, seglen=seglen,
                 kQ=fac(B, Hkv, T, rk) if rk else None, kP=fac(nseg, B, Hkv, D, rk) if rk else None,
                 vQ=fac(B, Hkv, T, rv) if rv else None, vP=fac(nseg, B, Hkv, D, rv) if rv else None)
    nblk = (T - seg0) // seglen if seglen else 0
    L = kk0 + nblk * kkb
    ko_t = np.full((B, Hkv, D, 2, L), -1, np.int64)
    ko_v = np.zeros((B, Hkv, D, 2, L))
    for b in range(B):
        for h in range(Hkv):
            for d in range(D):
                spans = [(0, seg0, kk0, 0)] + [(seg0 + j * seglen, seg0 + (j + 1) * seglen, kkb, kk0 + j * kkb) for j in range(nblk)]
                for lo, hi, k, at in spans:
                    if not k:
                        continue
                    tok = rng.choice(np.arange(lo, hi), size=2 * k, replace=False)
                    for side in (0, 1):
                        ko_t[b, h, d, side, at:at + k] = np.sort(tok[side * k:(side + 1) * k])
                        ko_v[b, h, d, side, at:at + k] = AP.f16((1 - 2 * side) * rng.uniform(2.5, 5.0, k))
    vo_c = np.full((B, T, 2, kv), -1, np.int64)
    vo_v = np.zeros((B, T, 2, kv))
    for b in range(B):
        for t in range(T):
            if kv:
                col = rng.choice(Hkv * D, size=2 * kv, replace=False)
                for side in (0, 1):
                    vo_c[b, t, side] = np.sort(col[side * kv:(side + 1) * kv])
                    vo_v[b, t, side] = AP.f16((1 - 2 * side) * rng.uniform(2.5, 5.0, kv))
    g16 = lambda m: AP.f16(rng.standard_normal((B, Hkv, m, D)))
    parts.update(ko_t=ko_t, ko_v=ko_v, vo_c=vo_c, vo_v=vo_v, kw=g16(W), vw=g16(W), kn=g16(n), vn=g16(n))
    return AP._finish(parts)


# name: (B, Hq, Hkv, T, W, n, bits, rk, rv, seg0, seglen, kk0, kkb, kv)
SHAPES = {
    "plain-T1024-W63-G4": (1, 8, 2, 1024, 63, 0, 2, 4, 4, 1024, 0, 10, 0, 3),
    "plain-T2112-W0-r0": (1, 2, 1, 2112, 0, 0, 4, 0, 0, 2112, 0, 12, 0, 0),
    "cache-T448-W17-rk4-rv8": (1, 4, 2, 448, 17, 0, 2, 4, 8, 192, 64, 4, 1, 2),
    "cache-R128-T512-W100-G3": (1, 3, 1, 512, 100, 0, 2, 8, 4, 256, 128, 3, 2, 2),
    "extend-G3-n37": (1, 3, 1, 320, 10, 37, 2, 8, 4, 128, 64, 3, 1, 2),
    "extend-G6-n45-W0": (1, 6, 2, 256, 0, 45, 4, 4, 4, 192, 64, 4, 1, 2),
    "extend-T0-n20": (1, 2, 1, 0, 30, 20, 2, 0, 0, 0, 64, 0, 0, 0),
}

# the mutations each shape must expose (a kind missing from mutation_sites fails test_every_applicable_mutation_has_a_site)
APPLIES = {name: [k for k in AP.MUTATIONS if
                  not (k.startswith("M2") and not s[5])
                  and not (k == "M2-gain-next" and s[5] < 2)
                  and not (k.startswith(("M3", "M6-k")) and not (s[11] or s[12]))
                  and not (k.startswith(("M4", "M6-v")) and not s[13])
                  and not (k in ("M4-v-head+1", "M4-v-head-1") and s[2] == 1)
                  and not (k == "M6-k-no-lr" and not s[7]) and not (k == "M6-v-no-lr" and not s[8])
                  and not (k.startswith("M5") and not (s[7] and s[10] and s[3] > s[9]))
                  and not (k == "M5-seg-1" and not (s[7] and s[10] and s[3] > s[9]))
                  and not (k == "M8-gqa-mod" and not (s[2] > 1 and s[1] > s[2]))
                  and not (k == "M7-no-rescale" and s[3] + s[4] + s[5] < 192 and s[3] < 128 and not (s[4] >= 2 and (s[3] or s[5])))]
           for name, s in SHAPES.items()}

_CACHE = {}


def _case(name):
    """(parts, Hq, rounds [(q [B,Hq,nq,D], probe row mask, exact (out, lse))], Kall, aimed) for a shape, built once."""
    if name not in _CACHE:
        B, Hq, Hkv, T, W, n, bits, rk, rv, seg0, seglen, kk0, kkb, kv = SHAPES[name]
        parts = synthetic_parts(sum(map(ord, name)), B, Hkv, T, W, n, bits, rk, rv, seg0, seglen, kk0, kkb, kv)
        rng = np.random.default_rng(7)
        kvx = AP.keys(parts)
        if n:
            qr, aimed = AP.extend_queries(parts, Hq, rng, kvx[0])
        else:
            qs, aimed = AP.decode_batches(parts, Hq, rng, kvx[0])
            q = np.concatenate(qs, axis=2)       # decode probes stacked as rows
            qr = [(q, np.ones(q.shape[:3], bool))]
        rounds = [(q, used, AP.ref(q, parts, kv=kvx)) for q, used in qr]
        _CACHE[name] = (parts, Hq, rounds, kvx, aimed)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_fp16_shaped_reference_within_a_third_of_the_bounds(name):
    parts, Hq, rounds, _, _ = _case(name)
    kv16 = AP.keys(parts, fp16=True)
    for q, _, (out, lse) in rounds:
        o16, l16 = AP.ref(q, parts, fp16=True, kv=kv16)
        r, e = AP.row_err(o16, out), AP.lse_err(l16, lse)
        assert r <= AP.ROW_BOUND / 3, r
        assert e <= AP.LSE_BOUND / 3, e


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_applicable_mutation_has_a_site(name):
    parts, Hq, _, _, aimed = _case(name)
    kinds = {k for k, _ in AP.mutation_sites(parts, Hq, aimed)}
    assert {w for k, w in AP.mutation_sites(parts, Hq) if k == "M1-drop"} <= aimed     # every standard M1 site has its probe
    assert kinds == set(APPLIES[name])


@pytest.mark.parametrize("name,kind", [(n, k) for n in SHAPES for k in APPLIES[n]], ids=[f"{n}-{k}" for n in SHAPES for k in APPLIES[n]])
def test_mutation_moves_the_probes_past_five_bounds(name, kind):
    parts, Hq, rounds, _, aimed = _case(name)
    sites = [w for k, w in AP.mutation_sites(parts, Hq, aimed) if k == kind]
    assert sites
    for where in sites:
        mp = AP.mutate(parts, kind, where)
        sig = 0.0
        for q, used, (out, lse) in rounds:
            rows = np.nonzero(used.any(axis=(0, 1)))[0]
            mo, ml = AP.ref(q[:, :, rows], mp, rows=rows)
            sig = max(sig, AP.signal(mo, ml, out[:, :, rows], lse[:, :, rows]))
        assert sig >= 5.0, (kind, where, sig)


@pytest.mark.parametrize("name", ["plain-T1024-W63-G4", "extend-G3-n37"])
def test_probe_families_each_dominated_by_their_targets(name):
    """Token / outlier / pair probes really are aimed: their targets hold all but e^-12 of the softmax mass."""
    parts, Hq, _, (Kall, _), _ = _case(name)
    rng = np.random.default_rng(3)
    fams = set()
    for qv, label, lo in AP.make_probes(parts, 0, 0, rng, Kall):
        fam = label.split("@")[0]
        fams.add(fam)
        if "@" not in label:
            continue
        tg = [int(x) for x in label.split("@")[1].split(".")[0].split("|")]
        s = Kall[0, 0] @ qv * AP.QSCALE
        rest = np.delete(s, tg)
        assert np.log(np.exp(s[tg] - s.max()).sum()) - np.log(np.exp(rest - s.max()).sum()) >= AP.DOMINANCE - 1e-9
    assert {"token", "k-outlier", "pair", "flat"} <= fams or not parts["ko_t"].size
