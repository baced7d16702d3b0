"""Prefix-snapshot timing (GPU box), one JSON line: the Llama-2-7B shape (32 layers, 32 KV heads), gearslKIVI 2-bit, rank 8, 2 %
outliers, one 4096-token prompt, batch 1, on a random-weight FastGearDecoder with shared_prefix_tokens = 4096:
  prefill_shared_ms   the dense prefill that stores the prompt (second run; the first warms up the GEMM / SDPA shapes)
  snapshot / restore  GearKVCachePool.snapshot() / .restore() of the prefix pool: one launch over the live bytes (`bytes`)
  torch_copy          the same state with torch: one copy_ per pool buffer at its full capacity (`bytes`), both directions
  host_round_trip     snap.cpu(pin_memory=True) and .to("cuda") of the blob
  load_prefix_ms      FastGearDecoder.load_prefix() of the prefix snapshot (restore + remainder rows + reset_shared)
Warm = median of 7 back-to-back calls; cold = median of 5 calls each behind a 512 MiB write.  Event times, us unless named ms.
usage: python tools/snapshot_timing.py [--layers N]   (--layers: fewer layers, debug only)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

dev = torch.device("cuda")
CC = dict(compress_method="gearslKIVI", group_size=64, residual=64, quantize_bit=2, rank=8, rankv=8, loop=3, left=0.02)


def timed(fn, flush=None):
    if flush is not None:
        flush.fill_(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3          # us


def measure(fn, flush):
    for _ in range(3):
        fn()
    return dict(warm=round(statistics.median(timed(fn) for _ in range(7)), 1),
                cold=round(statistics.median(timed(fn, flush) for _ in range(5)), 1))


def main():
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    layers = int(sys.argv[sys.argv.index("--layers") + 1]) if "--layers" in sys.argv else 32
    P = 4096
    mcfg = LlamaConfigLite(num_hidden_layers=layers, num_attention_heads=32, num_key_value_heads=32, hidden_size=4096,
                           intermediate_size=11008, max_position_embeddings=8192, k_bits=2, v_bits=2, group_size=64,
                           residual_length=64)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        torch.manual_seed(0)
        with torch.device(dev):
            model = LlamaForCausalLM_GEARKIVI(mcfg, CC).eval()
    finally:
        torch.set_default_dtype(old)
    ids = torch.randint(0, mcfg.vocab_size, (1, P), device=dev)
    flush = torch.empty((512 << 20) // 4, dtype=torch.float32, device=dev)
    make = lambda: FastGearDecoder(model, 128, batch=1, shared_prefix_tokens=P)
    warm = make()
    warm.prefill_shared(ids)
    del warm
    dec = make()
    res = dict(tool="snapshot_timing", gpu=torch.cuda.get_device_name(0), layers=layers, prompt=P,
               method="gearslKIVI 2-bit g64 rank 8, 2 % outliers")
    res["prefill_shared_ms"] = round(timed(lambda: dec.prefill_shared(ids)) / 1e3, 1)
    pool = dec.prefix_pool
    snap = pool.snapshot()
    full = sum(t.numel() * t.element_size() for t in pool.buf.values())
    res["bytes"] = dict(blob=snap.nbytes, buffers_full_capacity=full, fp16_kv=2 * layers * 32 * P * 128 * 2)
    res["snapshot_us"] = measure(lambda: pool.snapshot(), flush)
    res["restore_us"] = measure(lambda: pool.restore(snap), flush)
    clone = {k: torch.empty_like(t) for k, t in pool.buf.items()}

    def copy_out():
        for k, t in pool.buf.items():
            clone[k].copy_(t)

    def copy_in():
        for k, t in pool.buf.items():
            t.copy_(clone[k])
    res["torch_copy_out_us"] = measure(copy_out, flush)
    res["torch_copy_in_us"] = measure(copy_in, flush)
    res["torch_copy_launches"] = len(pool.buf)
    host = snap.cpu(pin_memory=True)
    res["host_round_trip_us"] = dict(to_host=measure(lambda: host.blob.copy_(snap.blob, non_blocking=True), flush),
                                     to_device=measure(lambda: host.to("cuda", non_blocking=True), flush))
    psnap = dec.snapshot("prefix")
    res["load_prefix_ms"] = round(statistics.median(timed(lambda: dec.load_prefix(psnap)) for _ in range(5)) / 1e3, 3)
    for n in ("snapshot_us", "restore_us"):
        res[n]["GBps_warm"] = round(2 * snap.nbytes / res[n]["warm"] / 1e3, 1)          # read + write
    print(json.dumps(res))


if __name__ == "__main__":
    from gear_amd import _lib
    _lib.load()
    main()
