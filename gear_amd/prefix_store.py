"""PrefixStore: a small least-recently-used store of prefix snapshots (FastGearDecoder.snapshot("prefix")), keyed by the exact
token ids of the prompt.  A server with several system prompts keeps them here and switches with load_prefix() -- a copy of the
compressed bytes -- instead of a prefill.  No prefix matching, no hashing beyond the ids tuple, no threading."""
from __future__ import annotations

from collections import OrderedDict

import torch


def _key(ids) -> tuple:
    if isinstance(ids, torch.Tensor):
        ids = ids.reshape(-1).tolist()
    return tuple(int(i) for i in ids)


class PrefixStore:
    def __init__(self, max_bytes: int, device: str = "cuda"):
        """max_bytes: the most the stored snapshots may hold together.  device: "cuda" keeps every snapshot where it was taken;
        "cpu" keeps it in host memory (one copy of the blob each way) and lookup() hands it back on the device it came from."""
        if device not in ("cuda", "cpu"):
            raise ValueError(f"PrefixStore: device {device!r}: 'cuda' or 'cpu'")
        if max_bytes < 0:
            raise ValueError(f"PrefixStore: max_bytes = {max_bytes}")
        self.max_bytes, self.device = int(max_bytes), device
        self._entries = OrderedDict()      # ids tuple -> (snapshot, the device it was taken on); least recently used first

    @property
    def bytes_used(self) -> int:
        return sum(s.nbytes for s, _ in self._entries.values())

    def __len__(self) -> int:
        return len(self._entries)

    def add(self, ids, snap):
        """Store `snap` under `ids` as the most recently used entry (replacing an entry of the same ids), evicting least recently
        used entries until it fits.  An entry larger than max_bytes is refused (ValueError) and the store is left as it was."""
        n = snap.nbytes
        if n > self.max_bytes:
            raise ValueError(f"PrefixStore.add: the snapshot holds {n} bytes, the store {self.max_bytes}")
        key = _key(ids)
        home = snap.device
        if self.device == "cpu":
            snap = snap.cpu()
        self._entries.pop(key, None)
        while self._entries and self.bytes_used + n > self.max_bytes:
            self._entries.popitem(last=False)
        self._entries[key] = (snap, home)

    def lookup(self, ids):
        """The snapshot stored under exactly these ids (marked most recently used), or None."""
        key = _key(ids)
        hit = self._entries.get(key)
        if hit is None:
            return None
        self._entries.move_to_end(key)
        snap, home = hit
        return snap if self.device == "cuda" or home.type == "cpu" else snap.to(home)
