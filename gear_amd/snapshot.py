"""Snapshots of the compressed cache: the live state of a GearKVCache / GearKVCachePool as ONE packed uint8 blob
(gear_cache_snapshot / gear_cache_restore, csrc/snapshot.hip) plus the few host-side values that give it meaning.

What a snapshot buys: a stored prompt can be taken out of a cache and put back -- or into another cache of the same geometry --
with one launch over its live compressed bytes instead of a dense prefill; the blob is one tensor, so moving it to host memory
and back is one copy each way.  The blob has no header: the counters (n_comp, n_win, seg0, kk0) that fix its layout travel in
the CacheSnapshot beside it, with a geometry key that a restore checks entry by entry before anything is written.

Generators.  The start bases of a block's low-rank factors are drawn for ALL batch rows at once from the pool's (or the cache's)
generator, so a generator state belongs to the whole batch, not to a sequence.  A whole-batch snapshot carries the states and a
whole-batch restore puts them back: what follows is bit-identical to what followed the snapshot.  A one-sequence restore (into
one slot, or broadcast to all) leaves the destination's generators alone: later blocks of such a fork follow the destination's
generator.

Nothing is cleared past the live ranges on restore: every compressed block, its outlier lists and its tiles are rewritten from
the live counters on and nothing reads past them (DESIGN.md "Shared-prefix extend" gives the argument for reset_shared(); the
restore relies on the same property)."""
from __future__ import annotations

import ctypes as C_

import torch

from . import _lib as L
from .cache import _state_view


def geometry_key(d: dict, H: int, D: int, mode: int = 0) -> dict:
    """What must agree between the cache a snapshot was taken from and the one it goes into: every entry of the cache dims (bits,
    group, residual, ranks, capacities, list and tile pitches), the KV heads, the head dimension and the arithmetic mode."""
    key = {k: int(v) for k, v in sorted(d.items())}
    key.update(H=int(H), D=int(D), mode=int(mode))
    return key


def _gen_state(g):
    return g.get_state().clone()


class CacheSnapshot:
    """blob: uint8 [nbytes], the packed live state of n_seq sequences of n_layers layers at the counters
    (n_comp, n_win, seg0, kk0); geometry: geometry_key() of the source; whole: taken with seq=None (then pool_gen / gens hold the
    generator states of the pool and of every per-layer cache; a one-sequence snapshot carries none)."""

    def __init__(self, blob, n_layers, n_seq, counters, geometry, whole, pool_gen=None, gens=()):
        self.blob = blob
        self.n_layers, self.n_seq = int(n_layers), int(n_seq)
        self.counters = tuple(int(c) for c in counters)
        self.geometry = dict(geometry)
        self.whole = bool(whole)
        self.pool_gen = pool_gen
        self.gens = list(gens)

    n_comp = property(lambda self: self.counters[0])
    n_win = property(lambda self: self.counters[1])
    seg0 = property(lambda self: self.counters[2])
    kk0 = property(lambda self: self.counters[3])
    device = property(lambda self: self.blob.device)

    @property
    def nbytes(self) -> int:
        return self.blob.numel()

    def _with_blob(self, blob):
        return self if blob is self.blob else CacheSnapshot(blob, self.n_layers, self.n_seq, self.counters, self.geometry, self.whole,
                                                            self.pool_gen, self.gens)

    def to(self, device, non_blocking: bool = False) -> "CacheSnapshot":
        """The snapshot with its blob on `device`: one copy (the generator states are small host tensors and stay where they are)."""
        return self._with_blob(self.blob.to(device, non_blocking=non_blocking))

    def cpu(self, pin_memory: bool = False) -> "CacheSnapshot":
        """The snapshot with its blob in host memory (pinned on request: .to("cuda", non_blocking=True) then overlaps)."""
        if self.blob.device.type == "cpu" and (not pin_memory or self.blob.is_pinned()):
            return self
        if not pin_memory:
            return self._with_blob(self.blob.cpu())
        host = torch.empty(self.blob.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(self.blob)
        return self._with_blob(host)

    def state_dict(self) -> dict:
        """Plain tensors, ints and containers of them: torch.save / torch.load round-trip it."""
        return dict(blob=self.blob, n_layers=self.n_layers, n_seq=self.n_seq, counters=list(self.counters),
                    geometry=dict(self.geometry), whole=int(self.whole), pool_gen=self.pool_gen, gens=list(self.gens))

    @classmethod
    def from_state_dict(cls, sd: dict) -> "CacheSnapshot":
        return cls(sd["blob"], sd["n_layers"], sd["n_seq"], sd["counters"], sd["geometry"], sd["whole"], sd.get("pool_gen"),
                   sd.get("gens", ()))


def check_compatible(snap, geometry: dict, n_layers: int, Tmax: int, R: int, what: str = "restore"):
    """Refuse a snapshot that does not fit the cache, before anything changes: ValueError naming the first differing geometry
    entry (or the layer count), GearError for more tokens than the capacity."""
    if not isinstance(snap, CacheSnapshot):
        raise ValueError(f"{what}: expected a CacheSnapshot, got {type(snap).__name__}")
    for k in sorted(set(geometry) | set(snap.geometry)):
        if geometry.get(k) != snap.geometry.get(k):
            raise ValueError(f"{what}: the snapshot was taken from a cache of another geometry: {k} = {snap.geometry.get(k)}, this "
                             f"cache has {k} = {geometry.get(k)}")
    if snap.n_layers != n_layers:
        raise ValueError(f"{what}: the snapshot holds {snap.n_layers} layers, this cache has {n_layers}")
    if snap.n_comp % 64 or min(snap.counters) < 0:
        raise L.GearError(f"{what}: the snapshot's counters (n_comp, n_win, seg0, kk0) = {snap.counters} are not a cache state: "
                          f"n_comp must be a multiple of 64 and no counter negative")
    if snap.n_comp > Tmax or snap.n_win > R:
        raise L.GearError(f"{what}: the snapshot holds {snap.n_comp} compressed + {snap.n_win} window tokens, the cache holds "
                          f"{Tmax} + {R}: capacity exceeded")


def _check_seq(seq, B, what):
    if seq is not None and (not isinstance(seq, int) or isinstance(seq, bool) or not 0 <= seq < B):
        raise ValueError(f"{what}: seq = {seq!r}: None or a sequence index in [0, {B})")


def _lockstep(caches, what):
    c0 = caches[0]
    if any((c.n_comp, c.n_win, c.seg0, c.kk0) != (c0.n_comp, c0.n_win, c0.seg0, c0.kk0) for c in caches):
        raise L.GearError(f"{what}: the layers' caches do not share one set of counters")
    return (c0.n_comp, c0.n_win, c0.seg0, c0.kk0)


def take(obj, bufs, d, n_layers, B, H, D, caches, pool_gen, seq) -> CacheSnapshot:
    """gear_cache_snapshot over `bufs` ([n_layers * B, ...] storage): all sequences (seq=None, with the generator states) or one."""
    _check_seq(seq, B, "snapshot")
    counters = _lockstep(caches, "snapshot")
    n_comp, n_win, seg0, kk0 = counters
    seq0, n_seq = (0, B) if seq is None else (seq, 1)
    dev = bufs["kwin"].device
    lib = L.load()
    view = _state_view(obj, bufs, d, n_layers * B, H, D, kk0, seg0)
    nbytes = lib.gear_cache_snapshot_bytes(C_.byref(view), n_layers, B, n_comp, n_win, n_seq)
    blob = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    if nbytes:
        L.require_gpu(blob)
        rc = lib.gear_cache_snapshot(C_.byref(view), n_layers, B, n_comp, n_win, seq0, n_seq, L.ptr(blob), nbytes,
                                     L.stream_ptr(blob))
        L.check(rc, "gear_cache_snapshot")
    whole = seq is None
    return CacheSnapshot(blob, n_layers, n_seq, counters, geometry_key(d, H, D), whole,
                         _gen_state(pool_gen) if whole and pool_gen is not None else None,
                         [_gen_state(c.gen) for c in caches] if whole else ())


def put(obj, bufs, d, n_layers, B, H, D, caches, pool_gen, snap, seq):
    """gear_cache_restore of `snap` into `bufs`.  Whole-batch snapshot + seq=None + equal batch: everything, counters and generator
    states included.  One-sequence blob (n_seq == 1) otherwise: seq=None broadcasts it to every sequence and sets the counters;
    seq=b writes slot b alone and needs the snapshot's counters to equal the current ones.  A whole snapshot of a batch-1 cache
    whose generator states do not fit this one (a standalone cache's into a pool, or the reverse) is such a one-sequence blob:
    it is broadcast and the generators are left alone; with more sequences that mismatch is refused.  All refusals come before
    any write."""
    check_compatible(snap, geometry_key(d, H, D), n_layers, d["Tmax"], d["R"])
    _check_seq(seq, B, "restore")
    gens_fit = len(snap.gens) == len(caches) and (pool_gen is not None) == (snap.pool_gen is not None)
    full = snap.whole and seq is None and snap.n_seq == B and (gens_fit or B != 1)
    if not full and snap.n_seq != 1:
        raise ValueError(f"restore: the snapshot holds {snap.n_seq} sequences: it restores a batch of {snap.n_seq} as a whole "
                         f"(seq=None; this cache has batch {B}); only a one-sequence snapshot goes into a slot or is broadcast")
    if seq is not None:
        now = _lockstep(caches, "restore")
        if now != snap.counters:
            raise ValueError(f"restore(seq={seq}): the snapshot's counters (n_comp, n_win, seg0, kk0) = {snap.counters} differ from "
                             f"the cache's {now}: the sequences of a cache advance in lockstep")
    if full and not gens_fit:
        raise ValueError("restore: the snapshot's generator states do not match this cache (pooled against standalone)")
    n_comp, n_win, seg0, kk0 = snap.counters
    seq0, n_seq = (0, B) if seq is None else (seq, 1)
    dev = bufs["kwin"].device
    lib = L.load()
    view = _state_view(obj, bufs, d, n_layers * B, H, D, kk0, seg0)
    need = lib.gear_cache_snapshot_bytes(C_.byref(view), n_layers, B, n_comp, n_win, snap.n_seq)
    if snap.nbytes != need:
        raise ValueError(f"restore: the blob has {snap.nbytes} bytes, this state takes {need}")
    if need:
        blob = snap.blob if snap.blob.device == dev else snap.blob.to(dev, non_blocking=True)
        L.require_gpu(blob)
        rc = lib.gear_cache_restore(C_.byref(view), n_layers, B, n_comp, n_win, seq0, n_seq, L.ptr(blob), need, snap.n_seq,
                                    L.stream_ptr(blob))
        L.check(rc, "gear_cache_restore")
    for c in caches:
        c.n_comp, c.n_win, c.seg0, c.kk0 = snap.counters
    if full:
        for c, st in zip(caches, snap.gens):
            c.gen.set_state(st)
        if pool_gen is not None:
            pool_gen.set_state(snap.pool_gen)


class DecoderSnapshot:
    """What FastGearDecoder.snapshot() returns.  what == "prefix": the stored prompt of a shared-prefix decoder -- the prefix
    pool's CacheSnapshot, the per-layer remainder rows and what reset_shared() restores (ids, logits row, pos, tail generator
    states).  what == "all": additionally the tail pool's CacheSnapshot, pos and shared_live (on a plain decoder: those alone)."""

    def __init__(self, what, prefix=None, shared_rem=None, saved=None, tail=None, pos=0, shared_live=False):
        self.what, self.prefix, self.shared_rem, self.saved = what, prefix, shared_rem, saved
        self.tail, self.pos, self.shared_live = tail, int(pos), bool(shared_live)

    def _tensors(self):
        out = [s.blob for s in (self.prefix, self.tail) if s is not None]
        for k, v in self.shared_rem or ():
            out += [k, v]
        if self.saved is not None:
            out += [self.saved["ids"], self.saved["logits"]]
        return out

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._tensors())

    @property
    def device(self):
        return self._tensors()[0].device

    def _map(self, blob_fn, small_fn):
        saved = None if self.saved is None else dict(self.saved, ids=small_fn(self.saved["ids"]), logits=small_fn(self.saved["logits"]))
        rem = None if self.shared_rem is None else [(small_fn(k), small_fn(v)) for k, v in self.shared_rem]
        return DecoderSnapshot(self.what, None if self.prefix is None else blob_fn(self.prefix), rem, saved,
                               None if self.tail is None else blob_fn(self.tail), self.pos, self.shared_live)

    def to(self, device, non_blocking: bool = False) -> "DecoderSnapshot":
        return self._map(lambda s: s.to(device, non_blocking), lambda t: t.to(device, non_blocking=non_blocking))

    def cpu(self, pin_memory: bool = False) -> "DecoderSnapshot":
        return self._map(lambda s: s.cpu(pin_memory), lambda t: t.cpu())

    def state_dict(self) -> dict:
        return dict(what=self.what, prefix=None if self.prefix is None else self.prefix.state_dict(),
                    shared_rem=None if self.shared_rem is None else [[k, v] for k, v in self.shared_rem], saved=self.saved,
                    tail=None if self.tail is None else self.tail.state_dict(), pos=self.pos, shared_live=int(self.shared_live))

    @classmethod
    def from_state_dict(cls, sd: dict) -> "DecoderSnapshot":
        cs = lambda x: None if x is None else CacheSnapshot.from_state_dict(x)
        rem = None if sd["shared_rem"] is None else [(k, v) for k, v in sd["shared_rem"]]
        return cls(sd["what"], cs(sd["prefix"]), rem, sd["saved"], cs(sd["tail"]), sd["pos"], sd["shared_live"])
