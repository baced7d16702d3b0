"""The admissible sets of tests/decomp_ref.py are (a) wide enough for a correct row decompressor and (b) narrow enough to catch the
faults they are for -- shown on the CPU, before any GPU run, on the very cases tests/test_gpu_decompress.py runs.

(a) A numpy float32 emulation of each accumulation order of csrc/decompress_rows_impl.h lands inside the set of every element of every
case: pairs onto the base (the v_dot2_f32_f16 chain), r sequential fmaf from zero and one add (the runtime-rank path), groups of four
onto the base in two orders (the matrix cores).  For rank 0 the reference equals the oracle's gears_tokenQ / gears_channelQ bit for
bit on a payload built with the oracle's own quantiser, and its dequantisation equals the oracle's in both scale arithmetics.

Measured (pytest -s prints every case): the largest share of elements with two admissible values is 2.18 % (asserted: at most 10 %),
and no element has more than two.

(b) Each fault of the list, injected into the emulation, is reported by `mismatches` (test_fault_is_reported)."""
import numpy as np
import pytest

import decomp_ref as R
from oracle import oracle as orc

F32, F64 = np.float32, np.float64
ORDERS = ("fdot2", "fmaf", "mfma_a", "mfma_b")


# ------------------------------------------------------------------------------------------------ float32 emulation of the kernel
def emulate(c, order, lr_at_outliers=True):
    """fp16 output of the case in the output layout, low-rank term added in float32 in the given order."""
    kind, r, k = c["kind"], c["r"], c["k"]
    base = R.base_values(c["code"], c["scale"], c["mn"], c["oidx"], c["oval"], kind, c["bits"], c["group"], c["mode"], c["B"], c["H"],
                         c["T"], R.HD, k)
    if r == 0:
        return base
    P, Q = np.asarray(c["P"], np.float16).astype(F32), np.asarray(c["Q"], np.float16).astype(F32)
    zero = np.zeros(base.shape, F32)

    def prod(ci):        # (exact in float32: two fp16 operands)
        if ci >= r:
            return zero
        if kind == "v":
            return Q[:, :, :, None, ci] * P[:, :, None, :, ci]
        return P[:, :, :, None, ci] * Q[:, :, None, :, ci]

    b32 = base.astype(F32)
    if order == "fdot2":
        acc = b32
        for c0 in range(0, r, 2):
            acc = (prod(c0) + prod(c0 + 1)) + acc
    elif order == "fmaf":
        acc = zero
        for ci in range(r):
            acc = (prod(ci).astype(F64) + acc.astype(F64)).astype(F32)
        acc = b32 + acc
    elif order == "mfma_a":
        acc = b32
        for c0 in range(0, r, 4):
            acc = acc + ((prod(c0) + prod(c0 + 1)) + (prod(c0 + 2) + prod(c0 + 3)))
    else:
        acc = b32
        for c0 in range(0, r, 4):
            acc = (((acc + prod(c0 + 3)) + prod(c0 + 2)) + prod(c0 + 1)) + prod(c0)
    out = acc.astype(np.float16)
    if not lr_at_outliers and k > 0:
        idx, _ = R.outlier_index(kind, c["oidx"], c["B"], c["H"], c["T"], R.HD)
        out[idx] = base[idx]
    return out


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_emulations_are_admissible_and_sets_are_small(name):
    c, sets = R.get_case(name)
    for order in ORDERS if c["r"] else ORDERS[:1]:
        R.assert_admissible(emulate(c, order), sets, "%s, %s" % (name, order))
    size = sets.size()
    share = float((size > 1).mean())
    print("%-48s %-34s two admissible values: %.3f %%, largest set %d" % (name, R.case_dispatch(c)["loop"], 100 * share, size.max()))
    assert size.min() >= 1 and size.max() <= 2 and share <= 0.10
    if c["r"] == 0:
        assert size.max() == 1


def test_worst_ambiguity_share():
    worst = max((float((R.get_case(n)[1].size() > 1).mean()), n) for n in R.CASE_NAMES)
    print("largest share of two-valued elements: %.3f %% (%s)" % (100 * worst[0], worst[1]))
    assert worst[0] <= 0.10


# ----------------------------------------------------------------------------------------------------------- against the oracle
def _oracle_payload(kind, x, bits, g, k):
    """A compressor-style payload built on the CPU with the oracle's selection and quantiser (fp32 arithmetic)."""
    B, H, T, D = x.shape
    rows = (R.to_rows("v", x) if kind == "v" else np.ascontiguousarray(x.transpose(0, 1, 3, 2)).reshape(B * H * D, T)).astype(F32)
    orig = rows.copy()
    isml, ilrg, mean = orc.outlier_select(rows, k)
    np.put_along_axis(rows, isml, mean[:, None], 1)
    np.put_along_axis(rows, ilrg, mean[:, None], 1)
    q = orc.quant_pack_lastdim(rows, g, bits, mode=1)
    oi = np.concatenate([np.sort(isml, 1), np.sort(ilrg, 1)], 1).astype(np.int64)
    ov = np.take_along_axis(orig, oi, 1).astype(np.float16)
    if kind == "v":
        lay = lambda a: np.ascontiguousarray(a.reshape(B, T, H, -1).transpose(0, 2, 1, 3))
    else:
        lay = lambda a: np.ascontiguousarray(a.reshape(B, H, D, -1))
    return lay(q["code"]), lay(q["scale"]), lay(q["mn"]), oi.astype(np.uint16), ov


@pytest.mark.parametrize("kind,bits", [("v", 2), ("v", 4), ("k", 2), ("k", 4)])
def test_rank0_reference_equals_the_oracle(kind, bits):
    B, H, T, D, g, k = 2, 2, 128, 128, 64, 3
    x = (np.random.default_rng(7).standard_normal((B, H, T, D)) * 1.5).astype(np.float16)
    code, scale, mn, oi, ov = _oracle_payload(kind, x, bits, g, k)
    got = R.decomp_sets(code, scale, mn, None, None, oi, ov, kind, bits, g, 1, B, H, T, D, 0, k)
    assert (got.size() == 1).all()
    s = 2.0 * k / (H * D) + 1e-9
    assert orc.outlier_count(B, H, T, D, s) == k
    want = orc.gears_tokenQ(x, bits, g, s) if kind == "v" else orc.gears_channelQ(x, bits, g, s).transpose(0, 1, 3, 2)
    R.assert_admissible(want, got, "oracle inside the reference's sets")
    base = R.base_values(code, scale, mn, oi, ov, kind, bits, g, 1, B, H, T, D, k)
    R.assert_bits(base, want, "reference base against the oracle")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bits", [2, 4, 8])
def test_dequantisation_equals_the_oracle(bits, mode):
    c = R.make_case("deq-%d-%d" % (bits, mode), "k", 1, 2, 256, bits=bits, mode=mode)
    got = R.base_values(c["code"], c["scale"], c["mn"], None, None, "k", bits, 64, mode, 1, 2, 256, R.HD, 0)
    R.assert_bits(got, orc.unpack_dequant_lastdim(c["code"], c["scale"], c["mn"], 64, bits, mode=mode), "dequantised values")


# -------------------------------------------------------------------------------------------------------------------- faults
def _fault_cases():
    return {"k": R.make_case("fault-k", "k", 1, 2, 1024, bits=2, r=8, k=3), "v": R.make_case("fault-v", "v", 2, 8, 128, bits=2, r=8, k=3)}


def _move_list(c, src, dst):
    oi, ov = c["oidx"].copy(), c["oval"].copy()
    if dst is not None:
        oi[dst], ov[dst] = oi[src], ov[src]
    oi[src], ov[src] = R.PAD, 0
    return dict(c, oidx=oi, oval=ov)


def _on_rows(c, out, fn):
    return R.from_rows(c["kind"], fn(R.to_rows(c["kind"], out)), c["B"], c["H"], c["T"], R.HD)


def _swap_store_halves(rows):
    """Lanes l and l + 32 exchange the wrong halves: columns 16 l + 8 .. 16 l + 15 against 16 (l + 32) .. 16 (l + 32) + 7."""
    rows = rows.copy()
    for l in range(32):
        a, b = slice(16 * l + 8, 16 * l + 16), slice(16 * (l + 32), 16 * (l + 32) + 8)
        rows[:, a], rows[:, b] = rows[:, b].copy(), rows[:, a].copy()
    return rows


def _one_ulp(c, out, sets):
    out = out.copy()
    idx = tuple(np.argwhere(sets.size() == 1)[1234])            # (an element with ONE admissible value: either neighbour is outside)
    out.view(np.uint16)[idx] += 1
    return out


def _dropped_entry(c):
    oi = c["oidx"].copy()
    oi[9, 0] = R.PAD
    return dict(c, oidx=oi)


FAULTS = {
    "factor row of the neighbouring token": lambda c: dict(c, Q=np.roll(c["Q"], -1, 2)),
    "factor row of the neighbouring channel": lambda c: dict(c, P=np.roll(c["P"], -1, 2)),
    "the neighbouring head's factor block": lambda c: dict(c, P=np.roll(c["P"], -1, 1), Q=np.roll(c["Q"], -1, 1)),
    "low-rank term dropped at outlier positions": "lr_at_outliers",
    "an outlier dropped": _dropped_entry,
    "an outlier list applied to the row above": lambda c: _move_list(c, 9, 8),
    "an outlier list applied to the row below": lambda c: _move_list(c, 9, 10),
    "outlier table shifted by one fill": lambda c: R.shifted_table(c, 4),
    "store halves of lanes l and l + 32 exchanged wrongly": ("out", lambda c, out, sets: _on_rows(c, out, _swap_store_halves)),
    "the next group's scale": R.next_group_scale,
    "mn of the next group": lambda c: dict(c, mn=np.roll(c["mn"], -1, -1)),
    "2-bit code pair swapped inside a byte": lambda c: dict(c, code=R.pack(R.unpack(c["code"], 2).reshape(-1, 2)[:, ::-1].reshape(
        R.unpack(c["code"], 2).shape), 2)),
    "block order permuted by a misplaced XCD remap": ("out", lambda c, out, sets: _on_rows(c, out, lambda rows: rows.reshape(
        -1, 16, rows.shape[1])[R.xcd_order(rows.shape[0] // 16)].reshape(rows.shape))),
    "one fp16 ulp on a single element": ("out", _one_ulp),
}


@pytest.fixture(scope="module")
def fault_cases():
    cases = _fault_cases()
    return {kind: (c, R.case_sets(c)) for kind, c in cases.items()}


@pytest.mark.parametrize("kind", ["k", "v"])
def test_the_fault_cases_pass_without_a_fault(fault_cases, kind):
    c, sets = fault_cases[kind]
    for order in ORDERS:
        R.assert_admissible(emulate(c, order), sets, order)


@pytest.mark.parametrize("kind", ["k", "v"])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_fault_is_reported(fault_cases, kind, fault):
    c, sets = fault_cases[kind]
    f = FAULTS[fault]
    for order in ("fdot2", "mfma_b"):
        if f == "lr_at_outliers":
            out = emulate(c, order, lr_at_outliers=False)
        elif isinstance(f, tuple):
            out = f[1](c, emulate(c, order), sets)
        else:
            out = emulate(f(c), order)
        n, lines = R.mismatches(out, sets)
        print("%s, %s, %s: %d elements reported" % (kind, fault, order, n))
        assert n > 0, (kind, fault, order)


def test_negative_control_references_differ():
    """The three wrong references of the GPU test's negative controls reject a correct output (here: the emulation)."""
    for name in R.NEGATIVE_CONTROLS:
        c, sets = R.get_case(name)
        out = emulate(c, "fdot2")
        assert R.mismatches(out, sets)[0] == 0
        d = R.case_dispatch(c)
        for what, wrong in (("lr", R.case_sets(c, lr_at_outliers=False)), ("table", R.case_sets(R.shifted_table(c, d["trows"]))),
                            ("scale", R.case_sets(R.next_group_scale(c)))):
            assert R.mismatches(out, wrong)[0] > 0, (name, what)


def test_subnormal_factor_cases_tell_kept_from_flushed():
    for name in R.SUBNORMAL_NAMES:
        c, kept = R.get_case(name)
        flushed = R.case_sets(c, flush=True)
        out = emulate(c, "fdot2")
        assert R.mismatches(out, kept)[0] == 0
        n = R.mismatches(out, flushed)[0]
        assert n > 0.5 * out.size, (name, n)
        assert (flushed.size() <= 2).all()


# ------------------------------------------------------------------------------------------------------- the dispatch table
def test_shapes_select_the_flavours_of_the_table():
    d = lambda kind, a, t, r=16, k=3, bits=2, **kw: R.dispatch(kind, bits, kw.pop("B", 1), a, t, r, k, **kw)
    for (h, t), rp in (((1, 128), 8), ((2, 64), 4), ((4, 32), 2)):
        x = d("v", h, t)
        assert (x["rpar"], x["rpb"], x["loop"]) == (rp, 16 * rp, "straight x%d" % rp)
        x = d("v", h, 40)
        assert (x["rpar"], x["rpb"], x["loop"]) == (rp, 8, "general")
    assert (d("v", 1, 17)["rpb"], d("v", 1, 17)["rpar"], d("v", 1, 17)["loop"]) == (1, 1, "general")
    x = d("v", 3, 16)
    assert (x["rpar"], x["threads"], x["loop"], x["swap"]) == (1, 64, "general", False)
    assert d("v", 8, 16)["loop"] == "straight" and d("v", 8, 16, r=8)["loop"] == "mfma16" and d("v", 8, 16, r=0)["loop"] == "straight"
    assert (d("v", 8, 16, r=5)["loop"], d("v", 8, 16, r=5)["arith"]) == ("general", "fmaf")
    assert d("v", 8, 16, bits=8)["loop"] == "general"
    assert d("v", 10, 16)["loop"] == "straight + general (last wave)" and d("v", 10, 16, r=4)["arith"] == "mfma + fdot2"
    assert d("v", 32, 16)["tb"] == 256 and d("v", 64, 16)["tb"] == 512 and d("v", 128, 16)["tb"] == 1024
    assert d("v", 64, 16)["shmem"] == 65536 > 48 * 1024 and d("v", 64, 16)["loop"] == "straight"
    assert (d("v", 128, 16)["trows"], d("v", 128, 16)["loop"]) == (2, "general")
    assert d("v", 32, 16, k=64)["pf_ok"] and not d("v", 32, 16, k=65)["pf_ok"] and d("v", 32, 16, k=65)["loop"] == "general"
    assert d("k", 2, 1024, k=16)["pf_ok"] and not d("k", 2, 1024, k=17)["pf_ok"] and d("k", 2, 1024, k=16)["loop"] == "straight"
    assert (d("k", 2, 16)["rpar"], d("k", 2, 64)["rpar"], d("k", 2, 16)["loop"]) == (64, 16, "general")
    assert d("k", 1, 640)["loop"] == "general" and d("k", 1, 1280)["loop"] == "straight + general (last wave)"
    assert d("k", 1, 8192, r=8)["loop"] == "mfma16" and d("k", 2, 16384, r=8)["loop"] == "general"
    for rpb in (32, 64, 128):
        assert d("k", 2, 1024, r=8, rpb_opt=rpb)["loop"] == "mfma rolled %d" % rpb
        assert d("v", 8, 128, r=4, rpb_opt=rpb, B=2)["loop"] == "mfma rolled %d" % rpb
        assert d("k", 2, 1024, r=8, rpb_opt=rpb, general=1)["loop"] == "general"
    assert d("k", 2, 1024, r=8, rpb_opt=-1)["loop"] == "mfma16"
    assert not d("k", 3, 1024, r=8, rpb_opt=128)["xcd"] and d("k", 8, 1024, r=8, rpb_opt=128)["xcd"]
    assert d("k", 3, 1024, r=8, rpb_opt=128)["nblocks"] == 3 and not d("k", 8, 1024, r=0, rpb_opt=128)["xcd"]


def test_the_cases_reach_every_flavour():
    seen = [dict(R.case_dispatch(R._SPECS[n]), **R._SPECS[n]) for n in R.CASE_NAMES]
    has = lambda **kw: any(all(s[a] == b for a, b in kw.items()) for s in seen)
    for loop in ("general", "straight", "straight x2", "straight x4", "straight x8", "mfma16", "mfma rolled 32", "mfma rolled 64",
                 "mfma rolled 128", "straight + general (last wave)", "mfma16 + general (last wave)"):
        for mode in (0, 1):
            assert has(loop=loop, mode=mode) or loop.startswith("mfma rolled") or "last wave" in loop, (loop, mode)
        assert has(loop=loop), loop
        for table in (False, True):
            assert any(s["loop"] == loop and (s["k"] > 0) == table for s in seen), (loop, table)
    for arith in ("none", "fmaf", "fdot2", "mfma", "mfma + fdot2"):
        for bits in (2, 4):
            assert has(arith=arith, bits=bits), (arith, bits)
    for kind in ("v", "k"):
        for tb in (256, 512, 1024):
            for r in (0, 16):
                assert has(kind=kind, tb=tb, r=r), (kind, tb, r)
            assert any(s["kind"] == kind and s["tb"] == tb and s["r"] in (4, 8) for s in seen)
            assert any(s["kind"] == kind and s["tb"] == tb and s["r"] in R.RUNTIME_RANKS for s in seen)
        assert sum(s["kind"] == kind and s["bits"] == 8 for s in seen) >= 2
        for mode in (0, 1):      # the fp16-arithmetic flavour with factors and outliers too
            assert any(s["kind"] == kind and s["mode"] == mode and s["r"] > 0 and s["k"] > 0 for s in seen)
    assert has(group=32) and has(group=128) and has(xcd=True, rpb=128) and has(kind="k", r=8, xcd=False, rpb=128)
    assert has(pf_ok=False, kind="v") and has(pf_ok=False, kind="k") and has(shmem=65536)
    assert has(flavour="cancel") and has(flavour="subnormal", arith="mfma") and has(flavour="subnormal", arith="fmaf")
