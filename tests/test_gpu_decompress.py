"""gear_decompress_rows (csrc/decompress_rows_impl.h) element by element against the float64 reference of tests/decomp_ref.py: every
output element must be one of the fp16 values the reference derives as admissible (one value for most elements, two near a rounding
boundary; rank 0: bit for bit) -- no scalar tolerance anywhere.  tests/test_decomp_ref_cpu.py shows on the CPU that a correct
decompressor passes these very cases, that each shape selects the flavour named below and that the faults the sets are for are caught.

The payloads are hand-built (decomp_ref.make_case): no compressor in the loop, outlier positions and values chosen.  Every case runs
twice: through the C entry with compress.decompress's argument list into a view of a larger allocation pre-filled with a NaN payload
(an element the kernel does not write, or a write outside the output, shows), and through compress.decompress itself, which must
return the same bytes.

Shape -> flavour (decomp_ref.dispatch restates the entry point's rules; V rows are H * 128 elements, K^T rows T elements):
  V H = 1 / 2 / 4, T = 128 / 64 / 32   8 / 4 / 2 rows side by side, sixteen straight-line steps
  V H = 1 / 2 / 4, T = 40              side by side, blocks of 8 rows: general loop
  V H = 1, T = 17                      one row per block
  V H = 3                              384 columns: a partial wave, no side by side, no store exchange
  V H = 8                              one full wave: straight-line (rank 0 / 16), matrix cores (rank 4 / 8), general loop (runtime rank)
  V H = 10                             second wave partial: straight-line first wave, general loop second
  V H = 32 / 64 / 128                  256 / 512 (64 KB table: raised dynamic-LDS limit) / 1024 threads (2-row table: general loop)
  K^T T = 16 / 64                      64 / 16 rows side by side, general loop
  K^T T = 640, 1280                    partial (last) wave
  K^T T = 1024 .. 8192                 whole waves, 256 / 512 threads; T = 16384: 1024 threads
  decomp_rpb 32 / 64 / 128             rank 4 / 8: the rolled loop over 4-row groups behind one factor-block load
  K^T T = 1024, 3 / 8 heads at 128 rows per block   XCD-contiguous block order off / on
  k = 16 | 17 (K^T T = 1024), 64 | 65 (V H = 32)    outlier entries prefetched one fill ahead | loaded inside the fill"""
import numpy as np
import pytest
import torch

import decomp_ref as R

pytestmark = pytest.mark.gpu
GUARD = 4096          # sentinel elements in front of and behind the output


@pytest.fixture(scope="module")
def env():
    from gear_amd import _lib as L
    from gear_amd import compress as C
    L.load()
    return C, L


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a.copy()).cuda()


def host(t):
    return t.cpu().numpy()


def payload_of(C, c):
    return C.Payload(c["kind"], (c["B"], c["H"], c["T"], R.HD), c["bits"], c["group"], c["mode"], dev(c["code"]), dev(c["scale"]),
                     dev(c["mn"]), dev(c["P"]), dev(c["Q"]), dev(c["oidx"]), dev(c["oval"]), c["k"])


def decompress_guarded(C, L, p):
    """compress.decompress's call (K: the K^T output) into a sentinel-filled view; asserts the guard regions stay untouched."""
    B, H, T, D = p.shape
    n = B * H * T * D
    alloc = torch.full((n + 2 * GUARD,), R.SENTINEL, dtype=torch.int16, device="cuda")
    out = alloc[GUARD:GUARD + n].view(torch.float16)
    lib = L.load()
    if p.kind == "v":
        rc = lib.gear_decompress_rows(L.ptr(p.code), L.ptr(p.scale), L.ptr(p.mn), B * T, T, H * T * D, D, H, D, T * D, p.group, p.bits,
                                      p.mode, 0, L.ptr(p.P), L.ptr(p.Q), p.rank, T, D, L.ptr(p.oidx), L.ptr(p.oval), p.k_out,
                                      out.data_ptr(), L.stream_ptr())
    else:
        rc = lib.gear_decompress_rows(L.ptr(p.code), L.ptr(p.scale), L.ptr(p.mn), B * H * D, D, D * T, T, 1, T, 0, p.group, p.bits,
                                      p.mode, 1, L.ptr(p.P), L.ptr(p.Q), p.rank, T, D, L.ptr(p.oidx), L.ptr(p.oval), p.k_out,
                                      out.data_ptr(), L.stream_ptr())
    L.check(rc, "gear_decompress_rows")
    torch.cuda.synchronize()
    assert bool((alloc[:GUARD] == R.SENTINEL).all()) and bool((alloc[GUARD + n:] == R.SENTINEL).all()), "write outside the output"
    return out.view(R.out_shape(p.kind, B, H, T, D))


def run_case(env, c):
    """fp16 output of the case (numpy, output layout) under the case's options."""
    C, L = env
    p = payload_of(C, c)
    L.set_option("decomp_rpb", c["rpb"])
    L.set_option("decomp_general", c["general"])
    try:
        got = decompress_guarded(C, L, p)
        again = C.decompress(p, transposed_out=True)
    finally:
        L.set_option("decomp_rpb", 0)
        L.set_option("decomp_general", 0)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), "compress.decompress returns other bytes than the guarded call"
    return host(got)


@pytest.mark.parametrize("name", [n for n in R.CASE_NAMES if n not in R.SUBNORMAL_NAMES])
def test_every_element_is_admissible(env, name):
    c, sets = R.get_case(name)
    got = run_case(env, c)
    R.assert_admissible(got, sets, "%s [%s]" % (name, R.case_dispatch(c)["loop"]))
    if c["r"] == 0:       # nothing is added: the bytes themselves, the sign of a zero included
        R.assert_bits(got, R.base_values(c["code"], c["scale"], c["mn"], c["oidx"], c["oval"], c["kind"], c["bits"], c["group"], c["mode"],
                                         c["B"], c["H"], c["T"], R.HD, c["k"]), name)


@pytest.mark.parametrize("name", R.SUBNORMAL_NAMES)
def test_subnormal_factor_entries_kept_or_flushed_whole(env, name):
    """Q all fp16 subnormals against P of +-2^13 .. 2^14: the term is of the base's size when the operands are honoured and zero when
    they are read as zero.  Each path must be one or the other for every element (DESIGN.md records which)."""
    c, kept = R.get_case(name)
    flushed = R.case_sets(c, flush=True)
    got = run_case(env, c)
    nk, lk = R.mismatches(got, kept)
    nf, lf = R.mismatches(got, flushed)
    d = R.case_dispatch(c)
    print("%s [%s, %s]: subnormal factor operands %s (outside the kept sets: %d, outside the flushed sets: %d of %d)" % (
        name, d["loop"], d["arith"], "kept" if nk == 0 else "flushed" if nf == 0 else "MIXED", nk, nf, got.size))
    assert nk == 0 or nf == 0, "neither kept nor flushed:\n" + "\n".join(lk + lf)


@pytest.mark.parametrize("name", R.NEGATIVE_CONTROLS)
def test_negative_controls_report_mismatches(env, name):
    """The GPU's output against three WRONG references: each must be rejected, or this file could not see that fault."""
    c, sets = R.get_case(name)
    assert c["guard"]
    got = run_case(env, c)
    R.assert_admissible(got, sets, name)
    wrong = {"low-rank term dropped at outlier positions": R.case_sets(c, lr_at_outliers=False),
             "outlier table shifted by one fill": R.case_sets(R.shifted_table(c, R.case_dispatch(c)["trows"])),
             "the next group's scale": R.case_sets(R.next_group_scale(c))}
    for what, ws in wrong.items():
        n, _ = R.mismatches(got, ws)
        print("%s, %s: %d elements reported" % (name, what, n))
        assert n > 0, what


@pytest.mark.parametrize("kind,H,T", [("v", 8, 64), ("k", 2, 1024)])
def test_compressor_made_payloads(env, kind, H, T):
    """The real layouts: compress_value / compress_key payloads (rank 8, 3 outliers a side, 2 bits) through the same check."""
    C, L = env
    torch.manual_seed(5)
    x = torch.randn(1, H, T, R.HD).half().cuda()
    P0 = torch.rand(1, H, R.HD, 8, device="cuda")
    comp = C.compress_value if kind == "v" else C.compress_key
    p = comp(x, 2, 64, k_out=3, rank=8, loop=3, mode="fp32", P0=P0)
    sets = R.decomp_sets(host(p.code), host(p.scale), host(p.mn), host(p.P), host(p.Q), host(p.oidx), host(p.oval), kind, 2, 64, p.mode,
                         1, H, T, R.HD, 8, 3)
    got = decompress_guarded(C, L, p)
    R.assert_admissible(host(got), sets, "compressor-made %s payload" % kind)
    a, b = C.decompress(p, transposed_out=True), C.decompress(p, transposed_out=False)
    assert torch.equal(a.view(torch.int16), got.view(torch.int16))
    if kind == "k":
        assert torch.equal(b.view(torch.int16), a.transpose(2, 3).contiguous().view(torch.int16))
    else:
        assert torch.equal(b.view(torch.int16), a.view(torch.int16))
