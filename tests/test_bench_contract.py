"""The bench.py output contract, checked on the bench line committed with the profiles (no GPU needed): the fields the
driver reads, the roofline and cpu_baseline objects, and internal consistency of the numbers."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


import pytest


@pytest.mark.parametrize("line", ["r1_final_bench_line.json", "r2_bench_line.json", "r3_bench_line.json", "r4_bench_line.json",
                                  "r5_bench_line.json"])
def test_committed_bench_line_has_the_contract_fields(line):
    d = json.load(open(os.path.join(ROOT, "profiles", line)))
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                     ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(d[key], typ), key
    assert "vs_baseline" in d and d["vs_baseline"] is None          # BASELINE.md publishes no number for this metric
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["scaling"] in ("weak", "strong")
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None or r["traffic"] >= 0.9 * r["alg_bytes_per_launch"]   # HBM bytes >= ~algorithmic bytes
    assert abs(r["achieved"] - r["alg_bytes_per_launch"] / (r["ms_per_launch"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == d["unit"] and c["sample"]
    # value = fp16 KV bytes through compress + decompress per second, whole job
    n = 32 * 32 * 4096 * 128
    assert abs(d["value"] - 2 * (2 * n * 2) / (d["ms_per_step"] * 1e-3) / 1e9) < 1e-6 * d["value"]
    if line.startswith(("r3", "r4", "r5")):
        # round 3 on: the headline roofline object is the compress CHAIN north_star names (the lower of K / V), with the PMC traffic of
        # its launches; the dominant single kernel rides along; the decode-time block boundary is measured and reported
        assert r["kernel"].startswith(("k_compress chain", "v_compress chain")) and "dominant_kernel" in r
        lo = min(d["roofline_chain"][c]["frac"] for c in ("k_compress", "v_compress"))
        assert abs(r["frac"] - lo) < 1e-12
        dk = r["dominant_kernel"]
        assert abs(dk["frac"] - dk["achieved"] / 8000.0) < 1e-9 and dk["ms_per_launch"] <= r["ms_per_launch"]
        bb = d["block_boundary"]
        assert bb["one_launch"] and 0 < bb["block_kernel_us"] < bb["chain_us"]
        assert abs(bb["frac"] - bb["alg_bytes"] / (bb["block_kernel_us"] * 1e-6) / 1e9 / 8000.0) < 1e-9
        assert bb["traffic"] is None or bb["traffic"] >= 0.9 * bb["alg_bytes"]
        assert abs(d["decode"]["block_compress_ms"] - bb["block_kernel_us"] * 1e-3) < 1e-9
        assert "numpy_glue" in c and c["value"] > c["numpy_glue"]["value"]
    if line.startswith("r5"):
        # round 5 (ADVICE): the untimed pre-warm is IN the line; bytes follow SURVEY 8(d) verbatim (4n/g for scale / mn,
        # 6 bytes per outlier) with the stored format beside them; the dominant kernel carries its duration alone AND inside the
        # two-stream step; the attention by batch stands beside an fp16-cache baseline; value vs stage timing is explained in the line
        assert d["prewarm_steps"] >= 0 and d["prewarm_s"] >= 0 and (d["prewarm_steps"] == 0) == (d["prewarm_s"] < 0.5)
        assert "timing_note" in d and "4n/g" in r["bytes_definition"] and "6 bytes per outlier" in r["bytes_definition"]
        v = d["roofline_chain"]["v_compress"]
        assert v["alg_bytes"] == 2 * n + n / 4 + 4 * n / 64 + 2 * 8 * (4096 + 128) * 1024 + 131072 * 80 * 6 and v["stored_bytes"] > v["alg_bytes"]
        dk = r["dominant_kernel"]
        assert dk["ms_per_launch_in_step"] is None or dk["ms_per_launch_in_step"] >= dk["ms_per_launch"]
        assert r["traffic"] is not None and r["traffic"] >= r["alg_bytes_per_launch"] and "r5_traffic.json" in r["traffic_source"]
        by_b = d["attn_decode"]["one_layer_streaming_cache_by_batch"]
        for b in ("B1", "B4", "B16"):
            assert by_b[b]["fp16_cache_us_per_call"] > 0
            assert abs(by_b[b]["speedup_vs_fp16_cache"] - by_b[b]["fp16_cache_us_per_call"] / by_b[b]["us_per_call"]) < 1e-9
        assert d["decode"]["hook_module_tokens_per_s"] >= 200.0
        # the reference harness's own comparison: the same decoder over an uncompressed fp16 cache, batch 1 and a serving batch
        vs = d["decode"]["vs_fp16_cache"]
        for b in ("B1", "B16"):
            assert vs[b]["gear_tokens_per_s"] > 0 and vs[b]["fp16_cache_tokens_per_s"] > 0 and vs[b]["gear_cache_MiB"] < vs[b]["fp16_cache_MiB"]
            assert abs(vs[b]["gear_vs_fp16_cache"] - vs[b]["gear_tokens_per_s"] / vs[b]["fp16_cache_tokens_per_s"]) < 1e-9
    if line.startswith("r4"):
        # round 4: the V chain is rows -> wave-private Gram kernel -> per-head solve -> Q pass; the PMC traffic of the chain is tied to
        # the library that produced the line; the hook module (the documented import swap) runs on its fast path
        assert r["traffic"] is not None and r["traffic"] >= r["alg_bytes_per_launch"]
        assert d["decode"]["hook_module_tokens_per_s"] >= 200.0
        assert d["decode"]["tokens_per_s"] >= d["decode"]["hook_module_tokens_per_s"] * 0.9
    if line.startswith("r2"):
        # round 2: per-kernel and per-chain rooflines on SURVEY 8(d) bytes (no error term), traffic tied to the library build
        assert "no error term" in r["bytes_definition"] and "traffic_source" in r
        for name in ("k_compress", "v_compress", "k_decompress", "v_decompress"):
            ch = d["roofline_chain"][name]
            assert abs(ch["frac"] - ch["alg_bytes"] / (ch["ms"] * 1e-3) / 1e9 / 8000.0) < 1e-9
        assert len(d["kernels"]) >= 3 and r["kernel"] in [kx["kernel"] for kx in d["kernels"]]
        assert abs(r["ms_per_launch"] - max(kx["ms"] for kx in d["kernels"][:3])) < 1e-12
        # 8(d) bytes of the V rows launch: read 2n + codes n/4 + scale / mn 8n/64 + 131072 rows x 80 entries x 4 bytes
        v = d["kernels"][0]
        assert v["kernel"].startswith("compress_rows_") and v["alg_bytes"] == 2 * n + n / 4 + 8 * n / 64 + 131072 * 80 * 4
        assert d["decode"]["outliers_per_side"]["v_row"] == 40 and "2% outliers" in d["decode"]["method"]


@pytest.mark.parametrize("name", ["r2_traffic.json", "r3_traffic.json", "r4_traffic.json", "r5_traffic.json", "r5c2_traffic.json"])
def test_traffic_profile_names_the_library_it_was_measured_on(name):
    t = json.load(open(os.path.join(ROOT, "profiles", name)))
    assert len(t["lib_sha256"]) == 64 and t["config"] == ("c2" if "c2" in name else "c3") and t["kernels"] and "FETCH_SIZE" in t["how"]
    if name.startswith("r5"):
        assert t["bench_step_avg_us"] and all(v > 0 for v in t["bench_step_avg_us"].values())
    assert all(v > 0 for v in t["kernels"].values())


def test_bench_parses_and_defaults_to_one_gpu():
    import ast
    src = open(os.path.join(ROOT, "bench.py")).read()
    ast.parse(src)
    assert '"--gpus", type=int, default=1' in src and '"--steps"' in src and '"--warmup"' in src


def test_round4_config2_line_is_committed_with_its_roofline():
    """BASELINE configs[1] (4-bit, rank 4, 1 % outliers, T = 2048): the 4-bit path has a measured line of its own."""
    d = json.load(open(os.path.join(ROOT, "profiles", "r4_bench_c2_line.json")))
    assert "T=2048" in d["config"]["workload"] and "4-bit" in d["config"]["workload"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    n = 32 * 32 * 2048 * 128
    assert abs(d["value"] - 2 * (2 * n * 2) / (d["ms_per_step"] * 1e-3) / 1e9) < 1e-6 * d["value"]
    for name in ("k_compress", "v_compress", "k_decompress", "v_decompress"):
        ch = d["roofline_chain"][name]
        assert abs(ch["frac"] - ch["alg_bytes"] / (ch["ms"] * 1e-3) / 1e9 / 8000.0) < 1e-9
    assert d["cpu_baseline"]["value"] > 0 and d["decode"]["tokens_per_s"] > 0


def test_sharded_line_reports_both_exchanges():
    """world > 1: the decode leg runs once per exchange -- the peer-store kernel (the build's default) and the all-gather collective
    north_star names -- and prints tokens/s for each (profiles/r4_bench_2rank_one_gpu.json: two ranks sharing ONE GPU over gloo, the
    control flow of `bench.py --gpus 2 --exchange both`; not a multi-GPU measurement)."""
    d = json.load(open(os.path.join(ROOT, "profiles", "r4_bench_2rank_one_gpu.json")))
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    modes = d["decode"]["exchange_modes"]
    assert set(modes) == {"peer", "collective"} and d["decode"]["exchange_default"] == "peer"
    for m in ("peer", "collective"):
        assert modes[m]["tokens_per_s"] > 0 and modes[m]["eager_tokens_per_s"] > 0 and modes[m]["exchange"]
    assert modes["peer"]["exchange_class"] == "PeerHeadGather" and modes["collective"]["exchange_class"] == "HeadGather"
    assert abs(d["decode"]["tokens_per_s"] - modes["peer"]["tokens_per_s"]) < 1e-6 * modes["peer"]["tokens_per_s"] + 30.0   # (MAX over ranks)
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"--exchange", default="both"' in src


def test_round5_sharded_lines_report_both_selections_and_shard_parity():
    """Sharded legs: `value` is the EXACT cross-shard V selection -- the algorithm of N = 1 --, the k / N per-shard
    selection stands beside it, and a start-up self-check compares the concatenated shard payloads with the unsharded payload.
    profiles/r5_emulation.jsonl: one rank's shard emulated on one GPU; profiles/r5_bench_2rank_one_gpu.json: two real ranks (gloo, both on
    one GPU: control flow, not a multi-GPU measurement), RCCL-style collective exchange first."""
    lines = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", "r5_emulation.jsonl"))]
    assert len(lines) == 6 and lines[0]["sharding"] is None
    for d in lines[1:]:
        sh = d["sharding"]
        assert sh["v_selection"] == "exact" and sh["shard_parity"] is True
        assert sh["per_shard"]["v_outliers_per_side"] <= sh["v_outliers_per_side"] and sh["per_shard"]["ms_per_step"] <= d["ms_per_step"] * 1.05
        assert abs(d["value_per_shard_selection"] - sh["per_shard"]["value_GBps"]) < 1e-9
    d = json.load(open(os.path.join(ROOT, "profiles", "r5_bench_2rank_one_gpu.json")))
    assert d["n_gpus"] == 2 and d["sharding"]["shard_parity"] is True and d["sharding"]["v_selection"] == "exact"
    assert d["decode"]["exchange_default"] == "collective" and set(d["decode"]["exchange_modes"]) == {"peer", "collective"}


def test_bench_plain_run_options(monkeypatch):
    """A plain run is the headline line only; --full adds the rest, --dump-outputs writes the last step's outputs, --steps >= 1."""
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 3 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_bench_dump_outputs_is_seeded_and_bounded(tmp_path):
    """--dump-outputs on host tensors of the payload layout (compress.py): float32 / float64 only, whole arrays below the per-array
    share of the budget, a seeded sample of the same positions above it, identical files from identical outputs, <= 64 MB."""
    import sys
    import numpy as np
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    from gear_amd.compress import Payload
    g = torch.Generator().manual_seed(0)
    L, H, T, D, r, k = 1, 4, 4096, 128, 8, 40

    def payload(kind, rows, per_row):
        return Payload(kind, (L, H, T, D), 2, 64, 1,
                       code=torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, per_row // 16), generator=g, dtype=torch.int32),
                       scale=torch.rand((rows, per_row // 64), generator=g), mn=torch.rand((rows, per_row // 64), generator=g),
                       P=torch.rand((L, H, D, r), generator=g).half(), Q=torch.rand((L, H, T, r), generator=g).half(),
                       oidx=torch.randint(0, 65535, (rows, 2 * k), generator=g, dtype=torch.int32).to(torch.uint16),
                       oval=torch.rand((rows, 2 * k), generator=g).half(), k_out=k)

    out = (payload("k", L * H * D, T), payload("v", L * H * T, D), torch.rand((L, H, D, T), generator=g).half(),
           torch.rand((L, H, T, D), generator=g).half())
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted([f"{kd}_{f}.npy" for kd in "kv" for f in ("code", "scale", "mn", "P", "Q", "oidx", "oval")] +
                           ["k_decompressed_t.npy", "v_decompressed.npy"])
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 64 << 20
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    P = np.load(tmp_path / "a" / "k_P.npy")                       # small: whole, in its shape
    assert P.shape == (L, H, D, r) and np.array_equal(P, out[0].P.float().numpy())
    kt = np.load(tmp_path / "a" / "k_decompressed_t.npy")        # 2M elements: the seeded sample
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(out[2].numel(), kt.size, replace=False))
    assert kt.size < out[2].numel() and np.array_equal(kt, out[2].reshape(-1).float().numpy()[idx])
    code = np.load(tmp_path / "a" / "v_code.npy")                # int32 code words: float64, exact
    assert code.dtype == np.float64 and np.array_equal(code, out[1].code.numpy().reshape(code.shape).astype(np.float64))
    u16 = [p.oidx.view(torch.int16).numpy().view(np.uint16) for p in out[:2]]     # positions above 2^15 included
    assert np.array_equal(np.load(tmp_path / "a" / "k_oidx.npy"), u16[0])            # whole
    oidx = np.load(tmp_path / "a" / "v_oidx.npy")                                    # sampled
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(u16[1].size, oidx.size, replace=False))
    assert oidx.size < u16[1].size and np.array_equal(oidx, u16[1].reshape(-1)[idx])
