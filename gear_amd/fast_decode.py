"""Fast single-token decode over GearKVCache: 6 launches per layer instead of the ~60 eager torch ops the attention
hook's forward issues per layer per token (cuda_supported_gear/modeling_llamagear.py:177-484 + decoder layer :502-560).

Takes the weights of a LlamaForCausalLM_GEARKIVI (any loader that fills that module works), fuses q/k/v and gate/up
projections into single GEMV weights, keeps the KV cache in GearKVCache (pre-allocated, kernel-native) and runs per layer
    [RMSNorm + qkv GEMV + RoPE + window append]  ->  fused attention over the compressed cache (2 launches)
    ->  [o_proj GEMV + residual add]  ->  [RMSNorm + gate/up GEMV + SwiGLU]  ->  [down GEMV + residual add]
with each bracketed group being one launch (gear_gemv_qkv_rope / gear_gemv_f16_add / gear_gemv_f16_norm) for batch <= 4;
larger batches use the library GEMM through torch.  Everything touching the cache is HIP.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib as L
from .cache import Fp16KVCache, GearKVCache, GearKVCachePool, KiviKVCache
from .modeling_llamagear import apply_rotary_pos_emb
from .rope import rope_parameters
from .logits import LogitsParams, TokenHistory, eos_ids, eos_update, process_logits
from .sampling import SamplingParams, sample_tokens


class FastGearDecoder:
    def __init__(self, model, max_tokens: int, batch: int = 1, seed: int = 0, tp_rank: int = 0, tp_world: int = 1,
                 tp_group=None, tp_exchange: str = "collective", v_selection: str = "exact", cache_kind: str = "gear",
                 shared_prefix_tokens: int = 0):
        """tp_world > 1: the cache and the attention are sharded head-wise: this rank owns
        Hq / tp_world query heads with their KV heads -- local q/k/v projection rows, local compressed cache, local attention --
        and all-gathers the per-rank attention output (parallel.HeadGather, pre-allocated) in front of the replicated
        o_proj / MLP, which every rank computes in full.  The model passed in holds the full (replicated) weights.
        tp_exchange: "collective" (default since round 5: the RCCL all-gather north_star names) = parallel.HeadGather
        (all_gather_into_tensor into a pre-allocated buffer; captured in the token-step graph when the RCCL capture probe passes),
        "peer" = parallel.PeerHeadGather (stores into the peers' hipIpc-mapped memory from one launch per layer, always capturable;
        falls back to the collective, on every rank alike, when the peer mappings cannot be set up).  Neither has run on more than
        one GPU yet (no multi-GPU node was ever available to this build): the collective is the conservative default.
        v_selection: "exact" = the V outliers of a token row are selected over ALL ranks' heads (the reference's row spans the heads:
        compress_function.py:304-311; csrc/vsel.hip through parallel.exact_v_thresholds: two launches + one small all-gather per
        compress call), "per_shard" = k / world inside the shard's own heads (rounds 1-3).
        cache_kind: "gear" (the compressed streaming cache) or "fp16" = cache.Fp16KVCache, the uncompressed baseline the reference's
        harness times beside the compressed models (cuda_supported_gear/test.py:41-62: model "None"): same weights, same fused GEMVs,
        same attention split / merge kernels over fp16 rows; eager steps on one GPU only.  "kivi" = cache.KiviKVCache, the KIVI
        baseline of that harness (modeling_llama_kivi.py's state machine: K block window, sliding fp16 V window) on csrc/kivi.hip --
        bits, group and residual length are the attention modules' (k_bits, group_size, residual_length), as the KIVI hook takes
        them; prefill / step / generate with eager steps on one GPU, everything else raises NotImplementedError.
        shared_prefix_tokens > 0: shared-prefix decoding -- `batch` sequences continue ONE prompt.  A second cache pool with batch 1
        and that capacity holds the prompt's compressed tokens once (same per-layer seeds: its payload is bit-identical to segment 0
        of a plain batch-1 decoder); `max_tokens` then sizes only the per-sequence tails.  prefill_shared() fills both, step() then
        attends through cache.attend_shared (gear_attn_decode_shared).  Eager steps on one GPU, compressed cache only.
        extend_shared() then feeds every sequence a chunk of its own behind the stored prompt (cache.attend_extend_shared), and
        reset_shared() returns the tails to their state after prefill_shared(): one stored prompt serves batch after batch."""
        self.model = model
        cfg = model.config
        self.cfg = cfg
        self.tp_rank, self.tp_world = tp_rank, tp_world
        self.Hq_full, self.Hkv_full = cfg.num_attention_heads, cfg.num_key_value_heads
        if self.Hq_full % tp_world or self.Hkv_full % tp_world:
            raise ValueError(f"{self.Hq_full} query / {self.Hkv_full} KV heads do not divide across {tp_world} ranks")
        self.Hq, self.Hkv = self.Hq_full // tp_world, self.Hkv_full // tp_world          # local heads
        self.D = cfg.hidden_size // cfg.num_attention_heads
        self.eps = cfg.rms_norm_eps
        self.theta = float(cfg.rope_theta)
        dev = model.lm_head.weight.device
        self.dev = dev
        # rope_scaling (linear / llama3 / yarn): the token step reads the frequencies from a device table (the gear_*_freq entry
        # points), the dense paths from the attention modules' ScaledRotaryEmbedding.  None: the theta code path, as before.
        # (Every rank of a sharded decoder computes the same table from the same config; captured graphs keep its pointer.)
        inv_freq, attn_factor = rope_parameters(cfg, self.D)
        self.rope = None if inv_freq is None else (inv_freq.to(dev).contiguous(), float(attn_factor))
        self.layers = []
        cc0 = model.model.layers[0].self_attn.compress_config
        # pooled cache storage: block boundaries compress every layer's window in one launch sequence
        if v_selection not in ("exact", "per_shard"):
            raise ValueError(f"v_selection {v_selection!r}: 'exact' or 'per_shard'")
        if cache_kind not in ("gear", "fp16", "kivi"):
            raise ValueError(f"cache_kind {cache_kind!r}: 'gear', 'fp16' or 'kivi'")
        if cache_kind == "fp16" and tp_world > 1:
            raise NotImplementedError("the fp16-cache baseline runs on one GPU")
        if cache_kind == "kivi" and tp_world > 1:
            raise NotImplementedError("the KIVI cache (cache_kind='kivi') runs on one GPU (tp_world > 1 is not implemented)")
        self.cache_kind = cache_kind
        if shared_prefix_tokens < 0:
            raise ValueError(f"shared_prefix_tokens = {shared_prefix_tokens}")
        if shared_prefix_tokens and cache_kind == "fp16":
            raise NotImplementedError("shared-prefix decoding is not implemented for the fp16-cache baseline (cache_kind='fp16')")
        if shared_prefix_tokens and cache_kind == "kivi":
            raise NotImplementedError("shared-prefix decoding is not implemented for the KIVI cache (cache_kind='kivi')")
        if shared_prefix_tokens and tp_world > 1:
            raise NotImplementedError("shared-prefix decoding is not implemented for head-sharded decoders (tp_world > 1)")
        self.shared_prefix_tokens = int(shared_prefix_tokens)
        self.shared_live = False      # prefill_shared() ran: step() attends over the stored prompt + the per-sequence tails
        self.prefix_pool = None
        self._shared_saved = None     # what reset_shared() restores: set by prefill_shared()
        tp = dict(rank=tp_rank, world=tp_world, group=tp_group, exact=v_selection == "exact") if tp_world > 1 else None
        self.pool = None if cache_kind != "gear" else GearKVCachePool(len(model.model.layers), batch, self.Hkv, max_tokens, cc0, dev,
                                                                      self.D, seed=seed, heads_total=self.Hkv_full, tp=tp)
        for i, layer in enumerate(model.model.layers):
            at, mlp = layer.self_attn, layer.mlp
            assert at.q_proj.bias is None, "attention_bias is not supported by the fused qkv GEMV"
            # RMSNorm weights are folded into the columns of the projection that follows them (the GEMV applies the
            # row scale rsqrt(mean(h^2) + eps) to its finished dot products), gate/up rows are interleaved so a GEMV
            # block finishes whole SwiGLU pairs
            n1, n2 = layer.input_layernorm.weight, layer.post_attention_layernorm.weight
            wqkv_full = torch.cat([at.q_proj.weight, at.k_proj.weight, at.v_proj.weight], 0) * n1[None, :]
            if tp_world > 1:
                D, r = self.D, tp_rank
                wqkv = torch.cat([at.q_proj.weight[r * self.Hq * D:(r + 1) * self.Hq * D],
                                  at.k_proj.weight[r * self.Hkv * D:(r + 1) * self.Hkv * D],
                                  at.v_proj.weight[r * self.Hkv * D:(r + 1) * self.Hkv * D]], 0) * n1[None, :]
            else:
                wqkv = wqkv_full
            wgu = torch.stack([mlp.gate_proj.weight, mlp.up_proj.weight], 1).reshape(-1, n2.shape[0]) * n2[None, :]
            self.layers.append(dict(
                wqkv=wqkv.contiguous(), wqkv_full=wqkv_full if tp_world > 1 else None, wo=at.o_proj.weight, wgu=wgu.contiguous(), wd=mlp.down_proj.weight,
                cache=(Fp16KVCache(batch, self.Hkv, max_tokens, dev, self.D) if cache_kind == "fp16" else
                       KiviKVCache(batch, self.Hkv, max_tokens, at.k_bits, at.group_size, at.residual_length, dev, self.D)
                       if cache_kind == "kivi" else
                       GearKVCache(batch, self.Hkv, max_tokens, at.compress_config, dev, self.D, seed=seed + i,
                                   pool=self.pool, layer=i, heads_total=self.Hkv_full, tp=tp)),
                rotary=at.rotary_emb))
        if self.shared_prefix_tokens:
            self.prefix_pool = GearKVCachePool(len(model.model.layers), 1, self.Hkv, self.shared_prefix_tokens, cc0, dev, self.D,
                                               seed=seed, heads_total=self.Hkv_full)
            for i, (lw, layer) in enumerate(zip(self.layers, model.model.layers)):
                lw["prefix"] = GearKVCache(1, self.Hkv, self.shared_prefix_tokens, layer.self_attn.compress_config, dev, self.D,
                                           seed=seed + i, pool=self.prefix_pool, layer=i, heads_total=self.Hkv_full)
        self.w_head = (model.lm_head.weight * model.model.norm.weight[None, :]).contiguous()
        self.pos = 0
        self.use_gemv = True
        self.batch = batch
        # hipGraph mode: device-side {pos, slot, T, W} shared by every layer's cache, static token / logits buffers
        self.state = torch.zeros(4, dtype=torch.int32, device=dev)
        for lw in self.layers:
            lw["cache"].state = self.state
        self.graph = None
        self.graph_sampled = None     # the sampled token step (step_graph_sampled) and the params it was captured with
        self._graph_sampling = None
        self.logits_sampled_static = None
        self.graph_proc = None        # the token step with logits processors / EOS bookkeeping (_generate_processed) and its key
        self._graph_proc_key = None
        self.logits_proc_static = None
        self._proc_state = None       # history, processed-logits buffer, done flags: the buffers that graph points at
        self._state_dirty = True      # host counters moved without the device-side state (eager step / prefill)
        self.tok = torch.zeros((batch, 1), dtype=torch.long, device=dev)
        self.logits_static = None
        self.gather = None
        self.exchange_error = None
        if tp_world > 1:
            from .parallel import HeadGather, PeerHeadGather
            if tp_exchange not in ("peer", "collective"):
                raise ValueError(f"tp_exchange {tp_exchange!r}: 'peer' or 'collective'")
            if tp_exchange == "peer":
                g = PeerHeadGather(tp_world, tp_rank, batch, self.Hq * self.D, torch.float16, dev, tp_group)
                if g.ok:
                    self.gather = g
                else:
                    self.exchange_error = g.error
            if self.gather is None:
                self.gather = HeadGather(tp_world, batch, self.Hq * self.D, torch.float16, dev, tp_group)

    def check_block_kernel(self):
        """Raise if a V tile of gear_compress_block ever gave up waiting for its row duties (csrc/block_fused.hip: the poll is
        bounded so that a shared / preempted GPU yields a status word instead of a hang; a tile that gave up has quantized with
        stale masks).  One device word: called every 16th block boundary and at the end of generate()."""
        from . import cache as gc
        st = gc.block_kernel_status(self.dev)
        if st:
            raise RuntimeError(f"gear_compress_block: hand-off timed out (status {st}); the cache contents since the last "
                               "check are not trustworthy -- set gear_amd.cache.USE_BLOCK_KERNEL = False to use the kernel chain")

    def _after_boundary(self):
        self._nbound = getattr(self, "_nbound", 0) + 1
        self.check_exchange()
        if self._nbound % 16 == 0:
            self.check_block_kernel()

    def check_exchange(self):
        """Sharded decoder: raise if the peer exchange ever timed out (one device word; called at block boundaries, at the end
        of generate() and by bench.py -- a latched timeout makes every later token silently wrong otherwise)."""
        if self.gather is not None and hasattr(self.gather, "check"):
            self.gather.check()

    def _attn_out(self, a):
        """[B, Hq_local, 1, D] of this rank -> [B, Hq_full * D] (all-gather over the head shards when sharded)."""
        a = a.view(a.shape[0], self.Hq * self.D)
        return a if self.gather is None else self.gather(a)

    # ------------------------------------------------------------------------------------------------ helpers
    def _fused(self, B, K):
        return self.use_gemv and B <= 4 and K % 8 == 0

    def _unit_rms(self, h):
        """RMSNorm without its weight (folded into the next projection), fp32 statistics like LlamaRMSNorm."""
        hf = h.float()
        return (hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + self.eps)).to(h.dtype)

    def _linear_add(self, x, w, res):
        """res + x @ w^T: the residual-stream update after o_proj / down_proj (gear_gemv_f16_add for B <= 4)."""
        B, K = x.shape
        if not self._fused(B, K):
            return res + F.linear(x, w)
        y = torch.empty_like(res)
        rc = L.load().gear_gemv_f16_add(L.ptr(x), L.ptr(w), B, K, w.shape[0], L.ptr(res), L.ptr(y), L.stream_ptr())
        L.check(rc, "gear_gemv_f16_add")
        return y

    def _norm_linear(self, res, w, swiglu=False):
        """RMSNorm(res) -> w (norm weight folded into w), optionally through SwiGLU (w rows interleaved).
        One launch (gear_gemv_f16_norm) for B <= 4; library GEMM otherwise."""
        B, K = res.shape
        N = w.shape[0]
        if self._fused(B, K):
            y = torch.empty((B, N // 2 if swiglu else N), dtype=res.dtype, device=res.device)
            rc = L.load().gear_gemv_f16_norm(L.ptr(res), None, None, self.eps, L.ptr(w), B, K, N, 1 if swiglu else 0,
                                             None, L.ptr(y), L.stream_ptr())
            L.check(rc, "gear_gemv_f16_norm")
            return y
        y = F.linear(self._unit_rms(res), w)
        return F.silu(y[:, 0::2]) * y[:, 1::2] if swiglu else y

    def _norm_qkv_rope(self, res, lw, dyn):
        """RMSNorm(res) -> fused q/k/v projection -> RoPE; k, v land in the cache window.  Returns q [B,Hq,1,128].
        dyn: position / slot come from the device state (graph replay)."""
        cache = lw["cache"]
        B, K = res.shape
        if self.cache_kind == "kivi":
            # the projection (one fused launch for B <= 4), then gear_kivi_rope_append: RoPE, K window, V ring and the evicted
            # V row's codes in one launch
            return cache.append_rope(self._norm_linear(res, lw["wqkv"]), self.Hq, self.pos, self.theta, rope=self.rope)
        if self._fused(B, K):
            if not dyn and cache.n_win >= cache.R:
                raise L.GearError(f"FastGearDecoder: the cache window is full ({cache.n_win} of {cache.R} slots): capacity reached")
            q = torch.empty((B, self.Hq, 1, self.D), dtype=res.dtype, device=res.device)
            head = (L.ptr(res), None, None, self.eps, L.ptr(lw["wqkv"]), B, K, self.Hq, self.Hkv, self.D,
                    0 if dyn else self.pos, 0 if dyn else cache.n_win, cache.R)
            tail = (L.ptr(self.state) if dyn else None, None, L.ptr(q), L.ptr(cache.kwin), L.ptr(cache.vwin), L.stream_ptr())
            if self.rope is None:
                rc = L.load().gear_gemv_qkv_rope(*head, self.theta, *tail)
                L.check(rc, "gear_gemv_qkv_rope")
            else:
                rc = L.load().gear_gemv_qkv_rope_freq(*head, L.ptr(self.rope[0]), self.rope[1], *tail)
                L.check(rc, "gear_gemv_qkv_rope_freq")
            if not dyn:
                cache.n_win += 1
            return q
        qkv = F.linear(self._unit_rms(res), lw["wqkv"])
        if dyn:
            return cache.append_rope_dyn(qkv, self.Hq, self.theta, rope=self.rope)
        return cache.append_rope(qkv, self.Hq, self.pos, self.theta, rope=self.rope)

    # ------------------------------------------------------------------------------------------------ prefill
    @torch.no_grad()
    def prefill(self, input_ids: torch.Tensor) -> torch.Tensor:
        """Dense causal attention over the prompt (torch SDPA), compress each layer's K/V into its cache.
        Returns the logits of the last position [B, vocab]."""
        return self._prefill(input_ids, False)

    @torch.no_grad()
    def prefill_shared(self, input_ids: torch.Tensor) -> torch.Tensor:
        """Shared-prefix prefill: ONE prompt input_ids [1, T] for all `batch` sequences.  The dense prefill runs at batch 1; the first
        T - T % residual tokens are compressed into the prefix caches (once), the T % residual remainder rows are copied into every
        sequence's window -- the tails' block boundaries then fall on the same absolute positions as in an unshared decoder.
        Returns the last position's logits repeated to [batch, vocab].  (A prompt shorter than `residual` has no compressed part:
        the tails hold all of it and step() attends over them alone.)"""
        if not self.shared_prefix_tokens:
            raise ValueError("prefill_shared(): construct the decoder with shared_prefix_tokens > 0")
        if input_ids.dim() != 2 or input_ids.shape[0] != 1 or input_ids.shape[1] < 1:
            raise ValueError(f"prefill_shared(): input_ids must be [1, T >= 1] (one prompt for all sequences), got "
                             f"{list(input_ids.shape)}")
        pc = self.layers[0]["prefix"]
        T = input_ids.shape[1]
        if T - T % pc.R > pc.Tmax:
            raise L.GearError(f"prefill_shared(): the prompt's compressed part ({T - T % pc.R} tokens) exceeds "
                              f"shared_prefix_tokens = {self.shared_prefix_tokens} (capacity {pc.Tmax})")
        logits = self._prefill(input_ids, True)
        # reset_shared() goes back to exactly this point: position, the tails' generator states (the remainder rows are kept per
        # layer by _store_prompt_shared); the ids and the logits row serve generate(reuse_prefix=True)
        self._shared_saved = dict(ids=input_ids.clone(), logits=logits, pos=self.pos, pool_gen=self.pool.gen.get_state(),
                                  gens=[lw["cache"].gen.get_state() for lw in self.layers])
        return logits.repeat(self.batch, 1)       # (rows of their own: the sampler takes no stride-0 rows)

    def reset_shared(self):
        """Return the decoder to its state right after prefill_shared() without touching the prefix pool: the tails are emptied
        (n_comp = seg0 = kk0 = 0), the prompt's T % residual remainder rows go back into every tail window, pos and the generator
        states of the tail pool and the per-layer tail caches are restored.  The stored prompt then serves the next batch: what
        that batch computes is bit-identical to the same batch on a fresh decoder (every compressed block, its outlier lists and
        its tiles are rewritten from position 0 on; nothing reads past the live counters)."""
        sv = self._shared_saved
        if sv is None:
            raise ValueError("reset_shared(): run prefill_shared() first")
        for lw, st in zip(self.layers, sv["gens"]):
            tc = lw["cache"]
            tc.n_comp = tc.seg0 = tc.kk0 = 0
            k, v = lw["shared_rem"]
            tc.n_win = k.shape[2]
            if tc.n_win:
                tc.kwin[:, :, :tc.n_win] = k
                tc.vwin[:, :, :tc.n_win] = v
            tc.gen.set_state(st)
        self.pool.gen.set_state(sv["pool_gen"])
        self.pos = sv["pos"]
        self._state_dirty = True

    def _kivi_refused(self, what):
        if self.cache_kind == "kivi":
            raise NotImplementedError(f"{what}: not implemented for the KIVI cache (cache_kind='kivi'): it has prefill(), eager "
                                      "step() and generate() only")

    @staticmethod
    def _logits_refused(what, logits):
        if logits is not None:
            raise NotImplementedError(f"{what}: logits processors (logits=LogitsParams) are not implemented here: they run in "
                                      "generate() only (eager steps on every cache kind, graph steps on the compressed cache)")

    def _shared_refused(self, what, hint=""):
        if self.shared_live:
            raise NotImplementedError(f"{what}: not implemented while a shared prefix is live (shared-prefix decoding has eager "
                                      f"step() / extend_shared() / generate(shared_prefix=True) only){hint}")

    def _store_prompt_shared(self, lw, k, v):
        """k, v [1, Hkv, T, 128] of the one prompt: compressed part -> the prefix cache, remainder rows -> every tail's window."""
        pc, tc = lw["prefix"], lw["cache"]
        assert tc.seq_len == 0
        T = k.shape[2]
        nq = T - T % pc.R
        if nq:
            pc.prefill(k[:, :, :nq], v[:, :, :nq])
        tc.n_win = T - nq
        lw["shared_rem"] = (k[:, :, nq:].clone(), v[:, :, nq:].clone())      # reset_shared() puts these few rows back
        if tc.n_win:
            tc.kwin[:, :, :tc.n_win] = k[:, :, nq:]
            tc.vwin[:, :, :tc.n_win] = v[:, :, nq:]

    def _prefill(self, input_ids, shared):
        B, T = input_ids.shape
        m = self.model.model
        h = m.embed_tokens(input_ids)
        pos = torch.arange(T, device=self.dev).unsqueeze(0)
        n_rep = self.Hq_full // self.Hkv_full
        for lw, layer in zip(self.layers, m.layers):
            # (the prompt is processed replicated, with every head; each rank keeps its own heads' K / V)
            wq = lw["wqkv"] if lw["wqkv_full"] is None else lw["wqkv_full"]
            qkv = F.linear(self._unit_rms(h), wq)              # input_layernorm's weight lives in wqkv's columns
            Hq, Hkv = self.Hq_full, self.Hkv_full
            q, k, v = qkv.split([Hq * self.D, Hkv * self.D, Hkv * self.D], dim=-1)
            q = q.view(B, T, Hq, self.D).transpose(1, 2)
            k = k.view(B, T, Hkv, self.D).transpose(1, 2)
            v = v.view(B, T, Hkv, self.D).transpose(1, 2)
            cos, sin = lw["rotary"](v, pos)
            q, k = apply_rotary_pos_emb(q, k, cos, sin)
            k0 = self.tp_rank * self.Hkv
            if shared:
                self._store_prompt_shared(lw, k, v)
            else:
                lw["cache"].prefill(k[:, k0:k0 + self.Hkv], v[:, k0:k0 + self.Hkv])
            kk = k if n_rep == 1 else k.repeat_interleave(n_rep, 1)
            vv = v if n_rep == 1 else v.repeat_interleave(n_rep, 1)
            a = F.scaled_dot_product_attention(q, kk, vv, is_causal=True)
            h = h + F.linear(a.transpose(1, 2).reshape(B, T, Hq * self.D), lw["wo"])
            h = h + layer.mlp(layer.post_attention_layernorm(h))
        self.pos = T
        self._state_dirty = True
        self.shared_live = bool(shared and self.layers[0]["prefix"].n_comp > 0)
        return self.model.lm_head(m.norm(h[:, -1]))

    # ------------------------------------------------------------------------------------------------ chunk extend
    @torch.no_grad()
    def extend(self, input_ids: torch.Tensor) -> torch.Tensor:
        """Feed n tokens [B, n] at once after prefill(): per layer the prefill-style dense projections, RoPE at pos .. pos + n - 1,
        chunk attention over the layer's cache (compressed part + window + the chunk itself, causal: cache.attend_extend), o_proj
        and MLP; then the tokens are committed (the windows fill, every `residual` tokens the pooled block compressor runs, exactly
        as n step() calls would run it).  Returns the logits of every position [B, n, vocab].
        More than N_MAX_EXTEND (2048) tokens go in pieces of that size, each committed before the next: a later piece sees the
        earlier ones as ordinary cache contents (compressed where a block boundary was crossed).  A call that would exceed the cache
        capacity is refused before anything changes."""
        from .cache import N_MAX_EXTEND, _check_room
        self._shared_refused("extend()", ": use extend_shared()")
        self._kivi_refused("extend()")
        if self.tp_world > 1:
            raise NotImplementedError("extend(): head-sharded (tp_world > 1) chunk extend is not implemented -- use step()")
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("extend(): chunk extend cannot be captured in a graph (host-side counters, block boundaries)")
        if self.pos == 0:
            raise ValueError("extend(): run prefill() first")
        if input_ids.dim() != 2 or input_ids.shape[0] != self.batch or input_ids.shape[1] < 1:
            raise ValueError(f"extend(): input_ids must be [{self.batch}, n >= 1], got {list(input_ids.shape)}")
        n = input_ids.shape[1]
        c0 = self.layers[0]["cache"]
        if self.pool is not None:
            _check_room(c0, n)
        elif c0.n_win + n > c0.R:
            raise L.GearError(f"extend(): {n} tokens after {c0.n_win} exceed the fp16 cache's capacity {c0.R}")
        out = [self._extend_piece(input_ids[:, i:i + N_MAX_EXTEND]) for i in range(0, n, N_MAX_EXTEND)]
        return out[0] if len(out) == 1 else torch.cat(out, 1)

    @torch.no_grad()
    def extend_shared(self, input_ids: torch.Tensor) -> torch.Tensor:
        """extend() behind a shared prefix: after prefill_shared(), feed every sequence n tokens of its own, input_ids [batch, n]
        (one n for all rows -- the sequences advance in lockstep; pad unequal messages to a common length).  Per layer the chunk
        attention runs over the stored prompt, the sequence's tail and the chunk itself (cache.attend_extend_shared: a prompt piece
        is reconstructed once per 64 query rows of any sequences, not once per decode step), then the tokens are committed to the
        tails as n step() calls would commit them.  Returns the logits of every position [batch, n, vocab].  More than
        N_MAX_EXTEND tokens go in committed pieces; a call that would exceed the tails' capacity is refused before anything
        changes.  A prompt shorter than `residual` has no compressed part: the chunk then runs over the tails alone."""
        from .cache import N_MAX_EXTEND, _check_room
        if self._shared_saved is None:
            raise ValueError("extend_shared(): run prefill_shared() first")
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("extend_shared(): chunk extend cannot be captured in a graph (host-side counters, block boundaries)")
        if input_ids.dim() != 2 or input_ids.shape[0] != self.batch or input_ids.shape[1] < 1:
            raise ValueError(f"extend_shared(): input_ids must be [{self.batch}, n >= 1], got {list(input_ids.shape)}")
        n = input_ids.shape[1]
        _check_room(self.layers[0]["cache"], n)
        out = [self._extend_piece(input_ids[:, i:i + N_MAX_EXTEND]) for i in range(0, n, N_MAX_EXTEND)]
        return out[0] if len(out) == 1 else torch.cat(out, 1)

    def _extend_piece(self, ids):
        B, n = ids.shape
        m = self.model.model
        h = m.embed_tokens(ids)
        pos = torch.arange(self.pos, self.pos + n, device=self.dev).unsqueeze(0)
        Hq, Hkv, D = self.Hq, self.Hkv, self.D
        ks, vs = [], []
        for lw, layer in zip(self.layers, m.layers):
            qkv = F.linear(self._unit_rms(h), lw["wqkv"])       # input_layernorm's weight lives in wqkv's columns
            q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
            q = q.view(B, n, Hq, D).transpose(1, 2)
            k = k.view(B, n, Hkv, D).transpose(1, 2)
            v = v.view(B, n, Hkv, D).transpose(1, 2).contiguous()
            cos, sin = lw["rotary"](v, pos)
            q, k = apply_rotary_pos_emb(q, k, cos, sin)
            q, k = q.contiguous(), k.contiguous()
            a = lw["cache"].attend_extend_shared(q, k, v, lw["prefix"]) if self.shared_live else lw["cache"].attend_extend(q, k, v)
            ks.append(k)
            vs.append(v)
            h = h + F.linear(a.transpose(1, 2).reshape(B, n, Hq * D), lw["wo"])
            h = h + layer.mlp(layer.post_attention_layernorm(h))
        if self.pool is not None:
            for _ in range(self.pool.extend_all(ks, vs)):
                self._after_boundary()
        else:
            for lw, k, v in zip(self.layers, ks, vs):
                lw["cache"].extend(k, v)
        self.pos += n
        self._state_dirty = True          # a later step_graph() brings the device-side state up to date
        return self.model.lm_head(m.norm(h))

    # ------------------------------------------------------------------------------------------------ speculative verify
    def _room(self) -> int:
        """The most tokens the caches can still take (extend() / verify() refuse more)."""
        c0 = self.layers[0]["cache"]
        if self.pool is None:
            return c0.R - c0.n_win
        return (c0.Tmax - c0.n_comp) // c0.R * c0.R + c0.R - 1 - c0.n_win

    @torch.no_grad()
    def verify(self, input_ids: torch.Tensor, logits=None) -> torch.Tensor:
        """Check n <= N_MAX_VERIFY (16) tokens [B, n] after prefill() without committing them: step()'s projections over B n rows
        (the fused GEMVs while B n <= 4), RoPE at pos .. pos + n - 1 and per layer cache.attend_verify (the decode kernels).  Returns the logits of every position [B, n, vocab]; every
        layer's n post-RoPE K / V rows are kept until accept(m) commits rows 0 .. m - 1.  Changes no cache state."""
        from .cache import N_MAX_VERIFY, _check_room
        self._logits_refused("verify()", logits)
        self._shared_refused("verify()")
        self._kivi_refused("verify()")
        if self.tp_world > 1:
            raise NotImplementedError("verify(): head-sharded (tp_world > 1) verification is not implemented -- use step()")
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("verify(): speculative verification cannot be captured in a graph (host-side counters)")
        if self.pos == 0:
            raise ValueError("verify(): run prefill() first")
        if input_ids.dim() != 2 or input_ids.shape[0] != self.batch or not 1 <= input_ids.shape[1] <= N_MAX_VERIFY:
            raise ValueError(f"verify(): input_ids must be [{self.batch}, n], 1 <= n <= {N_MAX_VERIFY} (longer chunks: extend()), "
                             f"got {list(input_ids.shape)}")
        B, n = input_ids.shape
        c0 = self.layers[0]["cache"]
        if self.pool is not None:
            _check_room(c0, n)
        elif c0.n_win + n > c0.R:
            raise L.GearError(f"verify(): {n} tokens after {c0.n_win} exceed the fp16 cache's capacity {c0.R}")
        self._pending = None
        m = self.model.model
        res = m.embed_tokens(input_ids).view(B * n, -1)          # the B n rows as step()'s batch rows
        pos = torch.arange(self.pos, self.pos + n, device=self.dev).unsqueeze(0)
        Hq, Hkv, D = self.Hq, self.Hkv, self.D
        ks, vs = [], []
        for lw in self.layers:
            # step()'s projections over B n rows: the fused GEMVs (one launch each) while B n <= 4, the library GEMM beyond
            qkv = self._norm_linear(res, lw["wqkv"]).view(B, n, -1)
            q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
            q = q.view(B, n, Hq, D).transpose(1, 2)
            k = k.view(B, n, Hkv, D).transpose(1, 2)
            v = v.reshape(B, n, Hkv, D).transpose(1, 2).contiguous()
            cos, sin = lw["rotary"](v, pos)
            q, k = apply_rotary_pos_emb(q, k, cos, sin)
            q, k = q.contiguous(), k.contiguous()
            a = lw["cache"].attend_verify(q, k, v)
            ks.append(k)
            vs.append(v)
            res = self._linear_add(a.transpose(1, 2).reshape(B * n, Hq * D), lw["wo"], res)
            act = self._norm_linear(res, lw["wgu"], swiglu=True)
            res = self._linear_add(act, lw["wd"], res)
        self._pending = dict(ks=ks, vs=vs, n=n, pos=self.pos)
        return self._norm_linear(res, self.w_head).view(B, n, -1)

    @torch.no_grad()
    def accept(self, m: int) -> int:
        """Commit rows 0 .. m - 1 (0 <= m <= n) of the last verify() to every layer's cache, exactly as extend() of those tokens
        commits them (the windows fill, the pooled block compressor runs at each boundary); advances pos.  Returns m."""
        self._shared_refused("accept()")
        self._kivi_refused("accept()")
        p = getattr(self, "_pending", None)
        if p is None or p["pos"] != self.pos:
            raise ValueError("accept(): no pending verify() (each verify() can be accepted once, before any other step)")
        if not 0 <= m <= p["n"]:
            raise ValueError(f"accept(): m = {m}, the last verify() checked n = {p['n']} tokens")
        self._pending = None
        if m == 0:
            return 0
        ks = [k[:, :, :m] for k in p["ks"]]
        vs = [v[:, :, :m] for v in p["vs"]]
        if self.pool is not None:
            for _ in range(self.pool.extend_all(ks, vs)):
                self._after_boundary()
        else:
            for lw, k, v in zip(self.layers, ks, vs):
                lw["cache"].extend(k, v)
        self.pos += m
        self._state_dirty = True          # a later step_graph() brings the device-side state up to date
        return m

    @torch.no_grad()
    def verify_tree(self, input_ids: torch.Tensor, parents: torch.Tensor, logits=None) -> torch.Tensor:
        """verify() over a draft tree: input_ids [B, n] are the nodes' tokens (node 0 = the last committed token), parents long [n]
        or [B, n] the tree (speculative.tree_layout's form, any device).  Node i runs at RoPE position pos + depth[b, i] and attends
        over the cache and its own ancestors among the n rows (cache.attend_verify_tree).  Returns the logits of every node
        [B, n, vocab]; every layer's n post-RoPE K / V rows and the parents are kept until accept_path(idx) commits one root path.
        verify()'s refusals; room is needed for the deepest path only.  Changes no cache state."""
        from .cache import N_MAX_VERIFY, _check_room
        from .speculative import tree_layout
        self._logits_refused("verify_tree()", logits)
        self._shared_refused("verify_tree()")
        self._kivi_refused("verify_tree()")
        if self.tp_world > 1:
            raise NotImplementedError("verify_tree(): head-sharded (tp_world > 1) verification is not implemented -- use step()")
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("verify_tree(): speculative verification cannot be captured in a graph (host-side counters)")
        if self.pos == 0:
            raise ValueError("verify_tree(): run prefill() first")
        if input_ids.dim() != 2 or input_ids.shape[0] != self.batch or not 1 <= input_ids.shape[1] <= N_MAX_VERIFY:
            raise ValueError(f"verify_tree(): input_ids must be [{self.batch}, n], 1 <= n <= {N_MAX_VERIFY}, "
                             f"got {list(input_ids.shape)}")
        B, n = input_ids.shape
        par = parents.detach().cpu()
        if par.shape[-1] != n or (par.dim() == 2 and par.shape[0] not in (1, B)):
            raise ValueError(f"verify_tree(): parents must be [{n}] or [{B}, {n}], got {list(parents.shape)}")
        anc, depth = tree_layout(par)                             # (on the host: n <= 16 nodes)
        deepest = int(depth.max()) + 1
        c0 = self.layers[0]["cache"]
        if self.pool is not None:
            _check_room(c0, deepest)
        elif c0.n_win + deepest > c0.R:
            raise L.GearError(f"verify_tree(): {deepest} tokens after {c0.n_win} exceed the fp16 cache's capacity {c0.R}")
        self._pending = self._pending_tree = None
        m = self.model.model
        res = m.embed_tokens(input_ids).view(B * n, -1)          # the B n rows as step()'s batch rows
        anc = anc.view(torch.int32).to(self.dev)
        pos = self.pos + depth.to(self.dev)
        Hq, Hkv, D = self.Hq, self.Hkv, self.D
        ks, vs = [], []
        for lw in self.layers:
            qkv = self._norm_linear(res, lw["wqkv"]).view(B, n, -1)
            q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
            q = q.view(B, n, Hq, D).transpose(1, 2)
            k = k.view(B, n, Hkv, D).transpose(1, 2)
            v = v.reshape(B, n, Hkv, D).transpose(1, 2).contiguous()
            cos, sin = lw["rotary"](v, pos)
            q, k = apply_rotary_pos_emb(q, k, cos, sin)
            q, k = q.contiguous(), k.contiguous()
            a = lw["cache"].attend_verify_tree(q, k, v, anc)
            ks.append(k)
            vs.append(v)
            res = self._linear_add(a.transpose(1, 2).reshape(B * n, Hq * D), lw["wo"], res)
            act = self._norm_linear(res, lw["wgu"], swiglu=True)
            res = self._linear_add(act, lw["wd"], res)
        self._pending_tree = dict(ks=ks, vs=vs, n=n, pos=self.pos, parents=par.reshape(-1, n).expand(B, n))
        return self._norm_linear(res, self.w_head).view(B, n, -1)

    @torch.no_grad()
    def accept_path(self, idx: torch.Tensor) -> int:
        """Commit one root path of the last verify_tree(): idx long [m] or [B, m], 0 <= m <= n, node indices root first (idx[:, 0]
        == 0, every next node a child of the one before -- checked on the host against the pending parents).  Those rows are
        gathered along the token axis and committed exactly as accept(m) commits rows 0 .. m - 1; advances pos.  Returns m.
        A verify_tree() is consumed by accept_path() only, a verify() by accept() only."""
        self._shared_refused("accept_path()")
        self._kivi_refused("accept_path()")
        p = getattr(self, "_pending_tree", None)
        if getattr(self, "_pending", None) is not None:
            raise ValueError("accept_path(): the pending pass is a verify(): commit it with accept()")
        if p is None or p["pos"] != self.pos:
            raise ValueError("accept_path(): no pending verify_tree() (each can be accepted once, before any other step)")
        B, n = p["parents"].shape
        ix = torch.as_tensor(idx).detach().cpu()
        if ix.dim() == 1:
            ix = ix.unsqueeze(0).expand(B, -1)
        if ix.dim() != 2 or ix.shape[0] != B or ix.dtype != torch.long or ix.shape[1] > n:
            raise ValueError(f"accept_path(): idx must be long [m] or [{B}, m], m <= {n}, got {list(ix.shape)} {ix.dtype}")
        m = ix.shape[1]
        if m:
            if bool((ix[:, 0] != 0).any()) or bool(((ix < 0) | (ix >= n)).any()) or \
                    not torch.equal(p["parents"].gather(1, ix[:, 1:]), ix[:, :-1]):
                raise ValueError("accept_path(): idx is no root path of the pending tree (idx[:, 0] == 0, parents[idx[:, j + 1]] "
                                 "== idx[:, j])")
        self._pending_tree = None
        if m == 0:
            return 0
        gx = ix.to(self.dev)[:, None, :, None].expand(B, self.Hkv, m, self.D)
        ks = [k.gather(2, gx) for k in p["ks"]]
        vs = [v.gather(2, gx) for v in p["vs"]]
        if self.pool is not None:
            for _ in range(self.pool.extend_all(ks, vs)):
                self._after_boundary()
        else:
            for lw, k, v in zip(self.layers, ks, vs):
                lw["cache"].extend(k, v)
        self.pos += m
        self._state_dirty = True          # a later step_graph() brings the device-side state up to date
        return m

    def _generate_tree(self, input_ids, max_length, n_draft, width, return_stats):
        """generate_speculative's loop over draft trees (tree_width > 1, the n-gram drafter, greedy acceptance)."""
        from .cache import N_MAX_VERIFY
        from .speculative import ngram_tree_draft, tree_accept
        n_draft = min(n_draft, N_MAX_VERIFY - 1)
        out = torch.cat([input_ids, self.prefill(input_ids).argmax(-1, keepdim=True)], 1)
        passes = drafted = accepted = 0
        while out.shape[1] < max_length:
            k = max(0, min(n_draft, max_length - out.shape[1] - 1, self._room() - 1))
            d, par = ngram_tree_draft(out, k + 1, width)
            nodes = torch.cat([out[:, -1:], d.to(out.dtype)], 1)
            lg = self.verify_tree(nodes, par)
            path, length, _ = tree_accept(nodes, par, lg)
            a = int(length.min()) - 1                               # the batch's minimum number of accepted drafts
            path = path[:, :a + 1]                                  # every row: its own path, cut to that length
            self.accept_path(path)
            # the argmax at the path's nodes = the row's accepted drafts, then the model's own token after them
            out = torch.cat([out, lg.argmax(-1).gather(1, path).to(out.dtype)], 1)
            passes += 1
            drafted += k
            accepted += a
        self.check_block_kernel()
        if not return_stats:
            return out
        gen = out.shape[1] - input_ids.shape[1]
        return out, dict(passes=passes, tokens=gen, tokens_per_pass=(gen - 1) / max(passes, 1), drafted=drafted, accepted=accepted,
                         acceptance_rate=accepted / max(drafted, 1))

    @torch.no_grad()
    def generate_speculative(self, input_ids: torch.Tensor, max_length: int, draft="ngram", n_draft: int = 3,
                             return_stats: bool = False, sampling=None, tree_width: int = 1, logits=None):
        """Greedy decoding with speculative verification: each pass drafts k <= n_draft tokens (draft = "ngram":
        speculative.ngram_draft over the tokens so far, or a callable (tokens [B, L], k) -> [B, k]), verifies [last token, d1 .. dk]
        in one verify() and commits the accepted drafts + the model's next token (accept(a + 1)).  With batch > 1 every row commits
        the batch's minimum accepted length a: the caches stay rectangular and every row's tokens stay the greedy ones (a row whose
        drafts ran longer re-proposes them next pass).  Returns [B, max_length] tokens as generate() does; with return_stats also
        dict(passes, tokens, tokens_per_pass, drafted, accepted, acceptance_rate).
        sampling (a sampling.SamplingParams): speculative sampling instead of greedy acceptance -- ONE gear_sample_tokens call over
        the verify logits [B, k + 1, V] accepts draft d_i with probability p(d_i) at its position and otherwise draws from p without
        d_i (the bonus row draws from p): every emitted token is an exact sample from the filtered distribution.  a = the batch
        minimum of leading accepts; a row that accepted further emits its draft at a, a row rejected at a its residual draw.
        tree_width > 1 (draft = "ngram", greedy only): every pass drafts a TREE of n_draft + 1 nodes (speculative.ngram_tree_draft:
        up to tree_width continuations of the trailing n-gram under one root), checks it in one verify_tree() pass, walks it with
        speculative.tree_accept and commits the batch's minimum path length through accept_path(), each row its own path."""
        from .speculative import accepted_lengths, ngram_draft
        self._logits_refused("generate_speculative()", logits)
        self._kivi_refused("generate_speculative()")
        if self.shared_prefix_tokens:
            raise NotImplementedError("generate_speculative(): not implemented for a shared-prefix decoder (shared_prefix_tokens > 0)")
        if tree_width > 1:
            if sampling is not None:
                raise NotImplementedError("generate_speculative(): sampling over a draft tree (tree_width > 1) is not implemented")
            if draft != "ngram" or n_draft < 0:
                raise ValueError(f"generate_speculative: tree_width = {tree_width} needs draft='ngram' and n_draft >= 0")
            return self._generate_tree(input_ids, max_length, n_draft, tree_width, return_stats)
        if tree_width < 1:
            raise ValueError(f"generate_speculative: tree_width = {tree_width}")
        if draft == "ngram":
            drafter = ngram_draft
        elif callable(draft):
            drafter = draft
        else:
            raise ValueError(f"generate_speculative: draft {draft!r}: 'ngram' or a callable (tokens, k) -> [B, k]")
        if n_draft < 0:
            raise ValueError(f"generate_speculative: n_draft = {n_draft}")
        from .cache import N_MAX_VERIFY
        n_draft = min(n_draft, N_MAX_VERIFY - 1)
        logits = self.prefill(input_ids)
        first = logits.argmax(-1, keepdim=True) if sampling is None else self._sample(logits, sampling)
        out = torch.cat([input_ids, first], 1)
        passes = drafted = accepted = 0
        while out.shape[1] < max_length:
            k = max(0, min(n_draft, max_length - out.shape[1] - 1, self._room() - 1))
            d = drafter(out, k) if k else out.new_zeros((out.shape[0], 0))
            d = d.to(device=out.device, dtype=out.dtype)
            if tuple(d.shape) != (out.shape[0], k):
                raise ValueError(f"generate_speculative: the drafter returned {list(d.shape)}, wanted [{out.shape[0]}, {k}]")
            lg = self.verify(torch.cat([out[:, -1:], d], 1))
            if sampling is None:
                a = int(accepted_lengths(d, lg).min())
                self.accept(a + 1)
                out = torch.cat([out, lg[:, :a + 1].argmax(-1)], 1)      # = the accepted drafts, then the model's own token
            else:
                # row i of a sequence predicts position pos + 1 + i; its draft is d_{i+1}, none (-1) for the bonus row
                B = out.shape[0]
                dr = torch.cat([d, d.new_full((B, 1), -1)], 1).reshape(-1).long()
                tok, acc, _ = sample_tokens(lg.reshape(B * (k + 1), -1), sampling, pos=self.pos + 1, n_per_seq=k + 1, draft=dr)
                tok, acc = tok.view(B, k + 1), acc.view(B, k + 1)
                a = int(acc[:, :k].long().cumprod(1).sum(1).min()) if k else 0
                self.accept(a + 1)
                out = torch.cat([out, tok[:, :a + 1].to(out.dtype)], 1)
            passes += 1
            drafted += k
            accepted += a
        self.check_block_kernel()
        if not return_stats:
            return out
        gen = out.shape[1] - input_ids.shape[1]
        return out, dict(passes=passes, tokens=gen, tokens_per_pass=(gen - 1) / max(passes, 1), drafted=drafted, accepted=accepted,
                         acceptance_rate=accepted / max(drafted, 1))

    # ------------------------------------------------------------------------------------------------ decode
    @torch.no_grad()
    def step(self, token_ids: torch.Tensor) -> torch.Tensor:
        """token_ids [B, 1] (or [B]) -> logits [B, vocab]; advances every layer's cache by one token."""
        m = self.model.model
        res = m.embed_tokens(token_ids.view(-1))            # [B, hidden]
        for lw in self.layers:
            cache = lw["cache"]
            q = self._norm_qkv_rope(res, lw, dyn=False)
            a = cache.attend_shared(q, lw["prefix"]) if self.shared_live else cache.attend(q)
            res = self._linear_add(self._attn_out(a), lw["wo"], res)
            act = self._norm_linear(res, lw["wgu"], swiglu=True)
            res = self._linear_add(act, lw["wd"], res)
        self.pos += 1
        self._state_dirty = True          # (the captured graph reads pos / slot / T / W from self.state)
        if self.pool is not None and self.layers[0]["cache"].n_win == self.layers[0]["cache"].R:
            self.pool.compress_all()
            self._after_boundary()
        elif self.cache_kind == "kivi":
            for lw in self.layers:
                lw["cache"].maybe_compress()      # the K window as one block, every `residual` tokens
        return self._norm_linear(res, self.w_head)

    # ------------------------------------------------------------------------------------------------ beam search
    def reorder(self, src_idx):
        """Sequence b continues from the history of sequence src_idx[b]: the per-sequence cache state of ALL layers is gathered along
        the batch axis in place, in one call (GearKVCachePool.reorder -> gear_cache_reorder).  src_idx: int32 / int64 device tensor
        [batch] (read on the device), a CPU tensor or a list.  With a shared prefix only the tails move -- the prefix pool is
        untouched; on a plain decoder the whole cache moves, prompt segment included (correct, only expensive)."""
        self._kivi_refused("reorder()")
        if self.tp_world > 1:
            raise NotImplementedError("reorder(): not implemented for head-sharded decoders (tp_world > 1)")
        if self.pool is None:
            raise NotImplementedError("reorder(): not implemented for the fp16-cache baseline (cache_kind='fp16')")
        self.pool.reorder(src_idx)
        self._state_dirty = True

    # ------------------------------------------------------------------------------------------------ snapshots
    def _snapshot_refused(self, what):
        self._kivi_refused(what)
        if self.tp_world > 1:
            raise NotImplementedError(f"{what}: not implemented for head-sharded decoders (tp_world > 1)")
        if self.pool is None:
            raise NotImplementedError(f"{what}: not implemented for the fp16-cache baseline (cache_kind='fp16')")

    def _prefix_parts(self):
        sv = self._shared_saved
        saved = dict(ids=sv["ids"].clone(), logits=sv["logits"].clone(), pos=sv["pos"], pool_gen=sv["pool_gen"].clone(),
                     gens=[g.clone() for g in sv["gens"]])
        rem = [(lw["shared_rem"][0].clone(), lw["shared_rem"][1].clone()) for lw in self.layers]
        return self.prefix_pool.snapshot(), rem, saved

    def snapshot(self, what: str = "all"):
        """The decoder's cache state as a snapshot.DecoderSnapshot (packed blobs: gear_cache_snapshot, one launch per pool).
        what="prefix" (a shared-prefix decoder after prefill_shared()): the stored prompt -- the prefix pool, the per-layer
        remainder rows and what reset_shared() restores (ids, logits row, pos, tail generator states): load_prefix() puts it into
        any decoder of the same model and configuration.  what="all": additionally the tails (the whole cache of a plain decoder),
        pos and shared_live: restore() resumes generation bit for bit where the snapshot was taken."""
        from .snapshot import DecoderSnapshot
        self._snapshot_refused("snapshot()")
        if what not in ("all", "prefix"):
            raise ValueError(f"snapshot(): what = {what!r}: 'all' or 'prefix'")
        has_prefix = self.prefix_pool is not None and self._shared_saved is not None
        if what == "prefix" and not has_prefix:
            raise ValueError("snapshot('prefix'): needs a shared-prefix decoder (shared_prefix_tokens > 0) after prefill_shared()")
        prefix, rem, saved = self._prefix_parts() if has_prefix else (None, None, None)
        if what == "prefix":
            return DecoderSnapshot("prefix", prefix, rem, saved)
        return DecoderSnapshot("all", prefix, rem, saved, self.pool.snapshot(), self.pos, self.shared_live)

    def _put_prefix(self, snap):
        """Prefix pool, remainder rows and _shared_saved from a snapshot that holds a stored prompt (checked before any write)."""
        from .snapshot import DecoderSnapshot
        if not isinstance(snap, DecoderSnapshot) or snap.prefix is None:
            raise ValueError("the snapshot holds no stored prompt (take it with snapshot('prefix') or snapshot('all') on a "
                             "shared-prefix decoder after prefill_shared())")
        if self.prefix_pool is None:
            raise ValueError("a stored prompt needs a shared-prefix decoder (shared_prefix_tokens > 0)")
        if len(snap.shared_rem) != len(self.layers) or len(snap.saved["gens"]) != len(self.layers):
            raise ValueError(f"the snapshot holds {len(snap.shared_rem)} layers, this decoder has {len(self.layers)}")
        self.prefix_pool.restore(snap.prefix)
        for lw, (k, v) in zip(self.layers, snap.shared_rem):
            lw["shared_rem"] = (k.to(self.dev), v.to(self.dev))
        sv = snap.saved
        self._shared_saved = dict(ids=sv["ids"].to(self.dev), logits=sv["logits"].to(self.dev), pos=int(sv["pos"]),
                                  pool_gen=sv["pool_gen"], gens=list(sv["gens"]))
        self._pending = None
        self._state_dirty = True

    def load_prefix(self, snap):
        """Make `snap`'s stored prompt this decoder's: the prefix pool, the remainder rows and the reset point are restored (one
        launch over the prompt's compressed bytes instead of a dense prefill), then reset_shared() empties the tails.  Works on a
        decoder in any state -- fresh, or in the middle of generation over another prompt.  Afterwards the decoder is in the state
        right after prefill_shared(ids): generate(ids, ..., shared_prefix=True, reuse_prefix=True), extend_shared() and
        generate_beam() go on from there."""
        self._snapshot_refused("load_prefix()")
        self._put_prefix(snap)
        self.shared_live = self.layers[0]["prefix"].n_comp > 0
        self.reset_shared()

    def restore(self, snap):
        """Return to a snapshot.  what="all": the tails (the whole cache of a plain decoder) with their counters and generator
        states, pos, shared_live and -- when it holds one -- the stored prompt: the steps that follow repeat, bit for bit, the
        steps that followed the snapshot.  what="prefix": load_prefix()."""
        from .snapshot import DecoderSnapshot, check_compatible, geometry_key
        self._snapshot_refused("restore()")
        if not isinstance(snap, DecoderSnapshot):
            raise ValueError(f"restore(): expected a DecoderSnapshot, got {type(snap).__name__}")
        if snap.what == "prefix":
            return self.load_prefix(snap)
        if snap.prefix is not None and self.prefix_pool is None:
            raise ValueError("restore(): the snapshot holds a stored prompt, this decoder has no prefix pool")
        p = self.pool                                           # the tails are checked before the stored prompt is written
        check_compatible(snap.tail, geometry_key(p.dims, p.H, p.D), p.L, p.dims["Tmax"], p.dims["R"], "restore()")
        if snap.tail.n_seq != p.B:
            raise ValueError(f"restore(): the snapshot holds {snap.tail.n_seq} sequences, this decoder has batch {p.B}")
        if snap.prefix is not None:
            self._put_prefix(snap)
        self.pool.restore(snap.tail)
        self.pos, self.shared_live = snap.pos, snap.shared_live
        self._pending = None
        self._state_dirty = True

    def generate_beam(self, input_ids: torch.Tensor, max_length: int, num_beams: int = None, eos_token_id: int = None,
                      length_penalty: float = 1.0, num_return_sequences: int = 1, pad_token_id: int = 0, logits=None):
        """Beam search with `batch` beams over ONE prompt input_ids [1, T] (a decoder built with shared_prefix_tokens > 0;
        num_beams, when given, must equal batch): prefill_shared() once, then per token log_softmax / top-2S in torch,
        reorder(beam_idx) and step().  Returns (sequences [num_return_sequences, max_length] long, padded with pad_token_id, scores
        [num_return_sequences] fp32: sum of log-probabilities / length ** length_penalty), best first.  The rule is fixed in
        gear_amd/beam.py.  Eager steps only."""
        from .beam import beam_search
        self._logits_refused("generate_beam()", logits)
        return beam_search(self, input_ids, max_length, num_beams, eos_token_id, length_penalty, num_return_sequences, pad_token_id)

    # ------------------------------------------------------------------------------------------------ hipGraph decode
    def _sync_state(self):
        c = self.layers[0]["cache"]
        self.state.copy_(torch.tensor([self.pos, c.n_win, c.n_comp, c.n_win + 1], dtype=torch.int32))

    def _step_body_dyn(self, sampling=None, proc=None):
        """The token step with every per-token scalar read from self.state on the device: identical launches for every
        token, so the whole thing (embedding -> 32 layers -> lm_head -> argmax -> state advance) is one graph.  With `sampling`
        the argmax is gear_sample_tokens at position state.pos + 1 (read on the device before the advance).  With `proc` (the
        state of _generate_processed) the token comes from the processed logits -- gear_logits_process with the history length
        state.pos + 1 and cur = the token just fed, appended inside the launch -- and gear_eos_update follows the choice."""
        m = self.model.model
        res = m.embed_tokens(self.tok.view(-1))
        for lw in self.layers:
            q = self._norm_qkv_rope(res, lw, dyn=True)
            a = lw["cache"].attend_dyn(q)
            res = self._linear_add(self._attn_out(a), lw["wo"], res)
            act = self._norm_linear(res, lw["wgu"], swiglu=True)
            res = self._linear_add(act, lw["wd"], res)
        logits = self._norm_linear(res, self.w_head)
        if proc is not None:
            src = logits
            if proc["lp"].active:
                src = process_logits(logits, proc["lp"], proc["hist"].buf, 1, proc["prompt_len"], cur=self.tok.view(-1),
                                     pos_dev=self.state, out=proc["buf"])
            self.tok.copy_(sample_tokens(src, proc["sp"], pos=1, pos_dev=self.state)[0].view(-1, 1))
            if proc["eos"]:
                eos_update(self.tok, proc["done"], proc["eos"], proc["pad"], proc["n_done"])
        elif sampling is None:
            self.tok.copy_(logits.argmax(-1, keepdim=True))
        else:
            self.tok.copy_(sample_tokens(logits, sampling, pos=1, pos_dev=self.state)[0].view(-1, 1))
        L.check(L.load().gear_decode_state_advance(L.ptr(self.state), L.stream_ptr()), "gear_decode_state_advance")
        return logits

    @torch.no_grad()
    def step_graph(self, token_ids: torch.Tensor = None) -> torch.Tensor:
        """One greedy decode token by replaying the captured graph.  token_ids (optional) overrides the token the graph
        produced itself; returns the NEXT token [B,1] (the graph's own argmax).  Block compression (every `residual`
        tokens) runs eagerly between replays."""
        return self._graph_step(token_ids, None)

    @torch.no_grad()
    def step_graph_sampled(self, sampling, token_ids: torch.Tensor = None) -> torch.Tensor:
        """step_graph() with gear_sample_tokens in place of the argmax: a graph of its own (self.graph_sampled, recaptured when
        `sampling` differs from the params it was captured with); the greedy graph is left alone.  Draws depend on (seed,
        sequence, position) only, so the tokens equal those of eager step() + sample_tokens at self.pos."""
        return self._graph_step(token_ids, sampling)

    def _graph_step(self, token_ids, sampling, proc=None):
        if self.shared_prefix_tokens:
            raise NotImplementedError("step_graph(): not implemented for a shared-prefix decoder (shared_prefix_tokens > 0): the "
                                      "shared-prefix attention has eager steps only")
        self._kivi_refused("step_graph()")
        if self.pool is None:
            raise NotImplementedError("step_graph(): the fp16-cache baseline has eager steps only")
        if self.gather is not None and not self.gather.capturable and not getattr(self, "_peer_tried", False):
            # the collective cannot be captured here (its probe failed, on every rank alike): a graph step needs the peer exchange
            # (csrc/xchg.hip, always capturable) -- set it up now, collectively, and keep the collective if that fails too
            self._peer_tried = True
            from .parallel import PeerHeadGather
            g = PeerHeadGather(self.tp_world, self.tp_rank, self.batch, self.Hq * self.D, torch.float16, self.dev,
                               getattr(self.gather, "group", None))
            if g.ok:
                self.gather = g
            else:
                self.exchange_error = g.error
        if self.gather is not None and not self.gather.capturable:
            raise NotImplementedError("step_graph() with tp_world > 1 needs a capturable exchange: tp_exchange='peer', or the "
                                      "collective on the RCCL backend when its capture probe passed (the one-GPU gloo staging "
                                      "path copies through the host) -- use step()")
        if token_ids is not None:
            self.tok.copy_(token_ids.view(self.batch, 1))
        if sampling is not None and self.graph_sampled is not None and self._graph_sampling != sampling:
            self.graph_sampled = None        # other params: capture again
        if proc is not None and self.graph_proc is not None and self._graph_proc_key != proc["key"]:
            self.graph_proc = None           # other params or other buffers: capture again
        graph = self.graph_proc if proc is not None else self.graph if sampling is None else self.graph_sampled
        if graph is None:
            self._sync_state()
            self._state_dirty = False
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                logits = self._step_body_dyn(sampling, proc)
            if proc is not None:
                self.graph_proc, self._graph_proc_key, self.logits_proc_static = graph, proc["key"], logits
            elif sampling is None:
                self.graph, self.logits_static = graph, logits
            else:
                self.graph_sampled, self._graph_sampling, self.logits_sampled_static = graph, sampling, logits
        elif self._state_dirty:          # an eager step() / prefill() ran since the last replay: bring the device state up to date
            self._sync_state()
        self._state_dirty = False
        graph.replay()
        self.pos += 1
        full = False
        for lw in self.layers:
            c = lw["cache"]
            c.n_win += 1
            full = c.n_win == c.R
        if full:
            self.pool.compress_all()
            self._sync_state()
            self._after_boundary()
        return self.tok

    def close(self):
        """Release the peer mappings of a sharded decoder (collective: every rank calls it)."""
        if self.gather is not None and hasattr(self.gather, "close"):
            self.gather.close()

    def _sample(self, logits, sampling):
        """The next token [B, 1] from logits [B, V] at position self.pos (the one after the last token fed)."""
        return sample_tokens(logits, sampling, pos=self.pos)[0].view(-1, 1)

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, max_length: int, graph: bool = False, sampling=None,
                 shared_prefix: bool = False, suffix_ids: torch.Tensor = None, reuse_prefix: bool = False,
                 return_logprobs: bool = False, logits=None, eos_token_id=None, pad_token_id=None, stop_check_every: int = 8):
        """Greedy decoding; with `sampling` (a sampling.SamplingParams) every token is drawn by gear_sample_tokens at its own
        position -- the first from the prefill logits, the rest from step()'s (graph=True: step_graph_sampled(), same tokens).
        shared_prefix=True (a decoder built with shared_prefix_tokens > 0): input_ids is ONE prompt [1, T], the result is
        [batch, max_length] -- `batch` continuations over the prompt stored once (prefill_shared()); the first token of every row
        comes from the one prefill row, sampled with the row index as the sampler's sequence index.
        suffix_ids [batch, n] (with shared_prefix): every sequence's own message behind the shared prompt -- prefill_shared(),
        then extend_shared(suffix_ids); the first token comes from the last extend row (sampler position T + n).  Rows of the
        result are prompt | suffix_s | generated, and max_length counts all of it.
        reuse_prefix=True (with shared_prefix): when a prompt is already stored, skip the prefill and reset_shared() instead --
        input_ids must be the stored prompt (ValueError otherwise).
        return_logprobs=True: returns (tokens, logprobs) -- logprobs fp32 [B, generated tokens], the log-softmax of each step's raw
        logits at the emitted token (before temperature / top-k / top-p: HF's compute_transition_scores on unprocessed scores),
        one gear_token_logprobs launch per step on the step's fp16 logits (graph=True: eagerly after each replay, on the graph's
        static logits buffer; the captured graphs are unchanged).  The tokens are those of the same call without it.
        logits (a logits.LogitsParams): every step's raw logits go through gear_logits_process (bias / bans, repetition penalty,
        n-gram ban, minimum length -- HF's processors in HF's order) into a buffer of their own, and the token is taken from that
        buffer by gear_sample_tokens (greedy = temperature 0: the first-index argmax); return_logprobs keeps reading the raw
        logits.  eos_token_id (an int or up to 8; default: logits.eos_token_id): gear_eos_update after every choice -- a row that
        emitted an EOS id is pad_token_id (default: the first EOS id) from then on, the host reads the count of finished rows every
        stop_check_every tokens (the one synchronisation this adds) and generation ends once every row is finished: the result
        is [B, L <= max_length], cut behind the last row's EOS as HF's generate() cuts it.  graph=True ("gear" cache): a graph of
        its own keyed by (sampling, logits, EOS ids, pad, buffers); the greedy and the sampled graph are left alone.  Without
        `logits` and `eos_token_id` nothing here runs."""
        if logits is not None and not isinstance(logits, LogitsParams):
            raise TypeError(f"generate(): logits must be a logits.LogitsParams, got {type(logits).__name__}")
        eos = eos_ids(eos_token_id) or (logits.eos_ids if logits is not None else ())
        if not eos and pad_token_id is not None:
            raise ValueError("generate(): pad_token_id without an eos_token_id")
        if not isinstance(stop_check_every, int) or stop_check_every < 1:
            raise ValueError(f"generate(): stop_check_every = {stop_check_every!r} must be an int >= 1")
        processed = bool(eos) or (logits is not None and logits.active)
        if processed and self.tp_world > 1:
            raise NotImplementedError("generate(logits= / eos_token_id=): not implemented for head-sharded decoders (tp_world > 1)")
        if shared_prefix and graph:
            raise NotImplementedError("generate(shared_prefix=True, graph=True): shared-prefix decoding has eager steps only")
        if graph or shared_prefix:
            self._kivi_refused("generate(graph=True)" if graph else "generate(shared_prefix=True)")
        if (suffix_ids is not None or reuse_prefix) and not shared_prefix:
            raise ValueError("generate(): suffix_ids / reuse_prefix need shared_prefix=True")
        lps = [] if return_logprobs else None      # one [B] column of log-probs per emitted token
        if processed:
            toks = self._generate_processed(input_ids, max_length, graph, sampling, logits or LogitsParams(), eos, pad_token_id,
                                            stop_check_every, shared_prefix, suffix_ids, reuse_prefix, lps)
            return (toks, torch.stack(lps, 1)) if return_logprobs else toks
        if sampling is not None:
            toks = self._generate_sampled(input_ids, max_length, graph, sampling, shared_prefix, suffix_ids, reuse_prefix, lps)
            return (toks, torch.stack(lps, 1)) if return_logprobs else toks
        logits, out = self._generate_start(input_ids, max_length, shared_prefix, suffix_ids, reuse_prefix)
        nxt = logits.argmax(-1, keepdim=True)
        self._record_logprobs(lps, logits, nxt)
        out.append(nxt)
        if graph and sum(t.shape[1] for t in out) < max_length:
            logits = self.step(nxt)                            # one eager step warms up every library handle
            nxt = logits.argmax(-1, keepdim=True)
            self._record_logprobs(lps, logits, nxt)
            out.append(nxt)
            self.tok.copy_(nxt)
        while sum(t.shape[1] for t in out) < max_length:
            if graph:
                nxt = self.step_graph().clone()
                self._record_logprobs(lps, self.logits_static, nxt)
            else:
                logits = self.step(nxt)
                nxt = logits.argmax(-1, keepdim=True)
                self._record_logprobs(lps, logits, nxt)
            out.append(nxt)
        self.check_exchange()
        self.check_block_kernel()
        toks = torch.cat(out, dim=1)
        return (toks, torch.stack(lps, 1)) if return_logprobs else toks

    @staticmethod
    def _record_logprobs(lps, logits, tok):
        """generate(return_logprobs=True): the log-prob of the emitted tokens tok [B, 1] under the step's raw logits [B, V]."""
        if lps is not None:
            from .scoring import token_logprobs
            lps.append(token_logprobs(logits, tok.reshape(-1)).logprobs)

    def score(self, input_ids: torch.Tensor, prompt_len: int, mode: str = "step", chunk: int = 512, top_k: int = 0):
        """Teacher-forced scoring of input_ids [B, T] on an empty decoder: prefill(input_ids[:, :prompt_len]), then the remaining
        tokens are fed and position t's log-prob is read from the logits that predict token t.  Returns a scoring.ScoreResult over
        the positions prompt_len .. T - 1 (logprobs, rank, nll, perplexity, top1; top_k > 0: the top log-probs of every position).
        mode="step": one step() per token -- every prediction sees exactly the cache a decoder would see at that point (the faithful
        measure of decode-time quality); every cache kind.  mode="extend": pieces of `chunk` tokens through extend() -- fast, but
        the tokens inside a piece see each other uncompressed; "gear" and "fp16" only (KIVI: extend()'s NotImplementedError).
        The decoder is left as the same prefill + step / extend calls leave it (the last token is a target only: T - 1 tokens
        are fed); a text that cannot fit is refused before anything changes.  The logits are read in place by gear_token_logprobs,
        one piece ([B, chunk, V] fp16) at a time: no fp32 copy, nothing wider than a piece."""
        from .scoring import score
        return score(self, input_ids, prompt_len, mode, chunk, top_k)

    def _generate_start(self, input_ids, max_length, shared_prefix, suffix_ids, reuse_prefix):
        """The prompt phase of generate(): (logits [B, vocab] the first token is taken from, the token columns so far)."""
        if not shared_prefix:
            return self.prefill(input_ids), [input_ids]
        if suffix_ids is not None and (suffix_ids.dim() != 2 or input_ids.shape[1] + suffix_ids.shape[1] >= max_length):
            raise ValueError(f"generate(): prompt ({input_ids.shape[1]}) + suffix {list(suffix_ids.shape)} leave no room for a "
                             f"generated token within max_length = {max_length}")
        sv = self._shared_saved
        if reuse_prefix and sv is not None:
            if input_ids.shape != sv["ids"].shape or not torch.equal(input_ids.to(sv["ids"].device), sv["ids"]):
                raise ValueError("generate(reuse_prefix=True): input_ids is not the prompt stored by prefill_shared()")
            self.reset_shared()
            logits = sv["logits"].repeat(self.batch, 1)
        else:
            logits = self.prefill_shared(input_ids)
        out = [input_ids.expand(self.batch, -1)]
        if suffix_ids is not None:
            logits = self.extend_shared(suffix_ids)[:, -1].contiguous()
            out.append(suffix_ids)
        return logits, out

    def _generate_sampled(self, input_ids, max_length, graph, sampling, shared_prefix=False, suffix_ids=None, reuse_prefix=False,
                          lps=None):
        logits, out = self._generate_start(input_ids, max_length, shared_prefix, suffix_ids, reuse_prefix)
        nxt = self._sample(logits, sampling)
        self._record_logprobs(lps, logits, nxt)
        out.append(nxt)
        if graph and sum(t.shape[1] for t in out) < max_length:
            logits = self.step(nxt)                             # one eager step warms up every library handle
            nxt = self._sample(logits, sampling)
            self._record_logprobs(lps, logits, nxt)
            out.append(nxt)
            self.tok.copy_(nxt)
        while sum(t.shape[1] for t in out) < max_length:
            if graph:
                nxt = self.step_graph_sampled(sampling).clone()
                self._record_logprobs(lps, self.logits_sampled_static, nxt)
            else:
                logits = self.step(nxt)
                nxt = self._sample(logits, sampling)
                self._record_logprobs(lps, logits, nxt)
            out.append(nxt)
        self.check_exchange()
        self.check_block_kernel()
        return torch.cat(out, dim=1)

    def _proc_begin(self, logits0, cap, sp, lp, eos, pad, prompt_ids):
        """The buffers of a processed generation: token history [B, cap] loaded with the prompt columns, the processed-logits
        buffer, the done flags and their count.  They are kept on the decoder while their shapes fit (the processed graph holds
        their pointers); its key names everything the capture bakes in."""
        B = logits0.shape[0]
        st = self._proc_state
        if st is None or st["hist"].cap != cap or st["buf"].shape != logits0.shape or st["buf"].dtype != logits0.dtype:
            st = dict(hist=TokenHistory(B, cap, self.dev), buf=torch.empty_like(logits0),
                      done=torch.zeros(B, dtype=torch.int32, device=self.dev), n_done=torch.zeros(1, dtype=torch.int32, device=self.dev))
            st["serial"] = getattr(self, "_proc_serial", 0) + 1
            self._proc_serial = st["serial"]
            self._proc_state = st
        st["done"].zero_()
        st["n_done"].zero_()
        n0 = st["hist"].load(prompt_ids)
        st.update(sp=sp, lp=lp, eos=eos, pad=pad, prompt_len=n0,
                  key=(sp, lp, eos, pad, n0 if lp.min_new_tokens else 0, st["serial"]))
        return st

    def _generate_processed(self, input_ids, max_length, graph, sampling, lp, eos, pad, every, shared_prefix=False, suffix_ids=None,
                            reuse_prefix=False, lps=None):
        """generate() with logits processors and / or EOS stopping: raw logits -> gear_logits_process -> gear_sample_tokens ->
        gear_eos_update per step; the history length is self.pos (every token fed so far), the token just fed is appended by the
        processing launch."""
        sp = sampling if sampling is not None else SamplingParams(temperature=0.0)
        pad = int(pad) if pad is not None else (eos[0] if eos else 0)
        logits, out = self._generate_start(input_ids, max_length, shared_prefix, suffix_ids, reuse_prefix)
        prompt = torch.cat([t.expand(logits.shape[0], -1) for t in out], 1)
        if prompt.shape[1] >= max_length:
            raise ValueError(f"generate(): the prompt ({prompt.shape[1]} tokens) leaves no room within max_length = {max_length}")
        st = self._proc_begin(logits, max_length, sp, lp, eos, pad, prompt)
        assert self.pos == st["prompt_len"], (self.pos, st["prompt_len"])

        def choose(raw, cur):
            src = raw
            if lp.active:
                src = process_logits(raw, lp, st["hist"].buf, self.pos, st["prompt_len"], cur=cur, out=st["buf"])
            tok = sample_tokens(src, sp, pos=self.pos)[0].view(-1, 1)
            if eos:
                eos_update(tok, st["done"], eos, pad, st["n_done"])
            return tok

        def finished(n_new):
            return bool(eos) and n_new % every == 0 and int(st["n_done"].item()) == st["done"].numel()

        nxt = choose(logits, None)
        self._record_logprobs(lps, logits, nxt)
        out.append(nxt)
        n_new, length = 1, prompt.shape[1] + 1
        if graph and length < max_length and not finished(n_new):
            logits = self.step(nxt)                             # one eager step warms up every library handle
            nxt = choose(logits, nxt.view(-1))
            self._record_logprobs(lps, logits, nxt)
            out.append(nxt)
            self.tok.copy_(nxt)
            n_new, length = n_new + 1, length + 1
        while length < max_length and not finished(n_new):
            if graph:
                nxt = self._graph_step(None, None, st).clone()
                self._record_logprobs(lps, self.logits_proc_static, nxt)
            else:
                logits = self.step(nxt)
                nxt = choose(logits, nxt.view(-1))
                self._record_logprobs(lps, logits, nxt)
            out.append(nxt)
            n_new, length = n_new + 1, length + 1
        self.check_exchange()
        self.check_block_kernel()
        toks = torch.cat(out, dim=1)
        if eos and int(st["n_done"].item()) == st["done"].numel():
            # every row is finished: cut behind the last row's EOS (its first EOS id among the generated tokens), as HF does
            hit = torch.isin(toks[:, prompt.shape[1]:], torch.tensor(eos, device=toks.device))
            keep = prompt.shape[1] + int(hit.int().argmax(1).max()) + 1
            toks = toks[:, :keep]
            if lps is not None:
                del lps[keep - prompt.shape[1]:]
        return toks
