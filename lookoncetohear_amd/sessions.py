"""The streaming drivers of `net.Net`: `Streamer` (one chunk per `step`, captured HIP graphs) and `SessionStreamer` (its
rows as listener slots that open, close, enroll, pause, move and fail one at a time), with the snapshots a session leaves
and comes back as.  `Net.make_streamer` / `Net.make_session_streamer` build them; `net` re-exports every name here."""
from __future__ import annotations

import ctypes
import math
from typing import TYPE_CHECKING, Optional

import numpy as np
import torch

from .weights import KV_PAD_ROWS, QK_PAD

if TYPE_CHECKING:
    from .net import Net


class Streamer:
    """8 ms-chunk streaming driver (reference usage: `Net.predict(chunk[B,2,192], embed[B,256], state, pad=False)`
    in a loop) with the per-chunk launch sequence captured once into HIP graphs.

    One chunk = 128 new samples + 64 look-ahead samples -> 128 output samples.  Everything the chunk loop touches is
    static device memory, and nothing is copied that a kernel can write in place:
      * conv / deconv / iSTFT tails and the inter-LSTM (h, c) exist twice; even chunks read set 0 and write set 1, odd
        chunks the other way round (two captured graphs, replayed alternately);
      * the K / V history of each block is a persistent 50-row ring in the attention kernel's own split-precision
        layout: the new row goes to slot (chunk mod 50) (`lh_qkv_proj_ln` ring_pos, a device counter the graph
        increments), and as the 50 rows are exactly the window of the chunk's one frame, nothing is ever moved;
      * the speaker gain LayerNorm(Linear(embedding)) is computed once in `set_embedding`.
    `step()` is: copy the chunk in, replay a graph, hand back the output buffer (a view that the next `step`
    overwrites).  `use_graph=False` runs the same launches eagerly (also what the capture warm-up does).
    `frames_per_chunk` = m in 1..16 (DESIGN.md §5 "Frames per chunk"): a chunk is m frames — 128 m new samples plus the 64 of
    look-ahead in, 128 m out — for hosts that can afford 8 m + 4 ms of algorithmic latency and want the per-chunk launch chain
    paid once per m frames.  The rings are then 49 + m rows; the m new rows go to slots pos .. pos + m - 1 (mod 49 + m) and the
    attention kernel reads the ring in place through a row map (`lh_local_attn_ring`), so still nothing is moved.  m = 1 is the
    object described above, launch for launch.
    Measured (MI355X, batch 1): 0.68 ms per chunk with the generic `predict` path captured in one graph, see DESIGN.md.
    """

    def __init__(self, net: Net, batch_size: int, device, use_graph: bool = True, frames_per_chunk: int = 1):
        if net.gemm_mode != "f16x3" or not net.fuse_linear:
            raise ValueError("Streamer runs the split-precision fused kernels (LOOKONCE_GEMM=f16x3, LOOKONCE_FUSE=1)")
        if isinstance(frames_per_chunk, bool) or not isinstance(frames_per_chunk, int) or not 1 <= frames_per_chunk <= 16:
            raise ValueError(f"frames_per_chunk must be an integer in 1..16 (one attention tile), got {frames_per_chunk!r}")
        self.net = net
        self.B = B = batch_size
        self.m = m = frames_per_chunk
        self.device = dev = torch.device(device)
        n = net.stft_chunk_size * m + net.stft_pad_size
        z = lambda *s, **k: torch.zeros(*s, device=dev, **k)
        self.chunk = z(B, net.num_ch, n)
        self.embed = z(B, net.spk_emb_dim)
        self.out = z(B, net.n_srcs, net.stft_chunk_size * m)
        F_, C_, nh, H_ = net.n_freqs, net.emb_dim, net.n_head, net.hidden
        mk = lambda: dict(conv_buf=z(B, net.num_ch * 2, 2, F_), deconv_buf=z(B, C_, 2, F_),
                          istft_buf=z(B, net.n_srcs, F_ * 2, 1),
                          h=[z(1, B * F_, H_) for _ in range(net.n_blocks)], c=[z(1, B * F_, H_) for _ in range(net.n_blocks)])
        self.sets = [mk(), mk()]
        rows = m + net.local_atten_len - 1 + KV_PAD_ROWS      # the ring is the first 49 + m of them, the rest stays zero
        self.rings = [(z(B * nh, rows, 2 * QK_PAD, dtype=torch.float16), z(B * nh, rows, 2 * net.V_dim * F_, dtype=torch.float16))
                      for _ in range(net.n_blocks)]
        self.pos = z(1, dtype=torch.int32)
        self.gain = z(B, F_, C_)
        self.gain_raw = z(B, F_ * C_)
        # range guard: THIS streamer's own two-word flag (never shared with the Net's offline forwards or another streamer);
        # a non-finite chunk (output: zeros) raises at the first `step` after that chunk has finished on the device.
        # On the GPU the flag lives in PINNED HOST memory (device-accessible under unified addressing): the back end stores
        # to it directly in the rare chunk that needs it and `step` just reads the word — no exchange kernel, no copy, no
        # extra launches in the chunk loop (round 3 polled with a kernel + copy every 64th chunk: +0.15 ms on that chunk,
        # which was the p99 of the latency distribution).
        self.range_flag = net._flag_words(dev)
        self.parity = 0
        self.graphs = None
        self.graph = None
        # strong references: the captured graphs bake in pointers into the packed weights and the T=1 workspace.
        # `Net._workspace` evicts its cache after a few shapes and `Net._weights` re-packs after any parameter change;
        # holding the objects here keeps the memory alive, and `step` refuses to replay once the weights were re-packed.
        with torch.no_grad(), net._device_ctx(self.chunk):
            self._pk = net._weights(dev)
            self._pack_key = net._pack_key
            self._n_steps = 0
            # (tensor, version at build time) of every parameter / buffer: `step` re-checks a few per chunk, round robin
            self._versions = [] if net._blob is not None else [(t, t._version) for t in list(net.parameters()) + list(net.buffers())]
            self._vpos = 0
            self._ws = net._workspace(B, m, dev)
            net._ws.pop((B, m, str(dev)), None)          # private to this streamer from now on
        if use_graph:
            self.graphs = self._capture(self._body, dev)
            self.graph = self.graphs[0]
            self.reset()

    @staticmethod
    def _capture(body, dev) -> list:
        """The two alternating per-chunk graphs of `body(k)`, k = 0, 1 (after one eager pass of each on a side stream)."""
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for k in (0, 1):                    # warm-up: packs weights, allocates the T=1 workspace
                body(k)
        torch.cuda.current_stream(dev).wait_stream(side)
        graphs = []
        for k in (0, 1):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body(k)
            graphs.append(g)
        return graphs

    def _body(self, k: int):
        with self.net._device_ctx(self.chunk):
            self.net._stream_chunk(self.chunk, self.gain, self.sets[k], self.sets[k ^ 1], self.rings, self.pos, self.out,
                                   self._pk, self._ws, self.range_flag)
            # ring slot counter, kept in [0, window): an ever-growing int32 would go negative after 2^31 chunks and C's
            # `%` would then index before the ring.  One 1-thread kernel (two torch elementwise launches cost 9 us of the chunk)
            st = self.net._stream(self.device)
            if self.m == 1:
                self.net._lib(self.pos).call("lh_ring_advance", self.pos.data_ptr(), self.net.local_atten_len, st)
            else:
                self.net._lib(self.pos).call("lh_ring_advance_by", self.pos.data_ptr(), self.m,
                                             self.net.local_atten_len - 1 + self.m, st)

    def _carried(self, k: int) -> list:
        """What a chunk carries in ping-pong set k: the conv / deconv / iSTFT tails, every block's h, every block's c."""
        x = self.sets[k]
        return [x["conv_buf"], x["deconv_buf"], x["istft_buf"]] + x["h"] + x["c"]

    def reset(self):
        for k in (0, 1):
            for t in self._carried(k):
                t.zero_()
        for kx, vx in self.rings:
            kx.zero_()
            vx.zero_()
        self.pos.zero_()
        self.range_flag.zero_()
        self.parity = 0

    def set_embedding(self, embed: torch.Tensor):
        self.embed.copy_(embed.reshape(self.B, -1))
        with torch.no_grad():
            self.net._speaker_gain(self.embed, self.gain_raw, self.gain)

    def step(self, chunk: torch.Tensor) -> torch.Tensor:
        """chunk [B, 2, 128 m + 64] (128 m new + 64 look-ahead samples) -> [B, 2, 128 m]."""
        if chunk.shape[-1] != self.chunk.shape[-1]:
            raise ValueError(f"a chunk of this streamer is {self.chunk.shape[-1]} samples "
                             f"({self.net.stft_chunk_size} x {self.m} new + {self.net.stft_pad_size} look-ahead), got {chunk.shape[-1]}")
        self._check_repacked()
        if self.net.range_check and int(self.range_flag[0]) != 0:     # host read of the pinned word: free
            self.range_flag.zero_()
            raise RuntimeError("LH_ERR_RANGE: an earlier chunk produced non-finite samples, emitted as zeros (inf / NaN in "
                               "the input or in the carried state); reset() the streamer")
        self._check_versions()
        self.chunk.copy_(chunk)
        with torch.no_grad():
            if self.graphs is not None:
                self.graphs[self.parity].replay()
            else:
                self._body(self.parity)
        self.parity ^= 1
        return self.out

    def _check_repacked(self):
        # O(1) staleness check (re-deriving the pack key walks all 130 parameters: ~0.1 ms of host time per 8 ms chunk):
        # any `Net` call after a parameter change re-packs and replaces `net._packed`.  The streamer owns references to
        # the images its graphs point into, so a stale streamer is never unsafe, only out of date.
        net = self.net
        cur = net._blob[1] if net._blob is not None else net._packed      # blob-only hosts (`from_packed`) never re-pack
        if cur is not self._pk:
            raise RuntimeError("the Net's parameters changed after this Streamer was built (its HIP graphs hold pointers "
                               "into the old packed weights): create a new streamer with net.make_streamer(...)")

    def _check_versions(self):
        # ... and a parameter updated IN PLACE (optimizer step, load_state_dict) without any other `Net` call in between
        # would replay silently on the old images: the tensors' version counters are re-checked three per chunk, round
        # robin (all ~130 within 0.4 s of audio).  Round 3 summed all of them every 64th chunk: ~0.13 ms of host time on
        # that chunk — exactly the p99 of the chunk latency (0.40 ms against a p50 of 0.26).
        self._n_steps += 1
        for _ in range(3 if self._versions else 0):
            t, v = self._versions[self._vpos]
            self._vpos = (self._vpos + 1) % len(self._versions)
            if t._version != v:
                raise RuntimeError("a parameter of the Net was modified in place after this Streamer was built: create a new "
                                   "streamer with net.make_streamer(...)")


class _Span(ctypes.Structure):
    """`lh_span_t` (include/lookonce_hip.h): one tensor of per-slot streaming state."""
    _fields_ = [("base", ctypes.c_void_p), ("bytes", ctypes.c_ulonglong)]


def _cuda_device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _copy_behind(data: torch.Tensor, event, dev: torch.device):
    """`data` copied into the memory of GPU `dev` behind `event`, without waiting: (the copy, an event behind it)."""
    if data.is_cuda:                                        # the copy is issued on the source's current stream
        cur = torch.cuda.current_stream(data.device)
        if event is not None:
            cur.wait_event(event)
        data.record_stream(cur)
    data = data.to(dev, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    return data, ev


class SessionSnapshot:
    """One listener's streaming state as a value: what `SessionStreamer.suspend` takes out and `resume` puts back, into any
    slot of any `SessionStreamer` of the same model — after a minute, on another GPU, in another process.
    `data`: ONE contiguous uint8 tensor in the layout of include/lookonce_hip.h ("suspend / resume"): header, the words, the
    speaker embedding, the tails and (h, c) of the live ping-pong set, the 50 window rows per head of every K / V ring.
    `event`: recorded behind the kernel that filled `data` (None for host memory, or where nothing is in flight); a resume on
    another stream orders itself behind it with a stream wait.  `layout`: the header's sizes on the host, so that `resume`
    can refuse a snapshot of another model without reading device memory.
    A snapshot is never written after it was filled: it can be resumed any number of times.  The state is only meaningful
    under the weights it was computed with; nothing checks that.  `to` never waits for the device; `cpu`, `save` and `load`
    may: they are not for the chunk loop."""
    MAGIC, VERSION, HEADER_BYTES = 0x5353484c, 1, 256       # LH_SNAPSHOT_*
    batch, index = None, 0                                  # a view of a `SessionSnapshotBatch`: the batch and the row

    def __init__(self, data: torch.Tensor, layout: tuple, event=None):
        self.data, self.layout, self.event = data, tuple(layout), event

    @staticmethod
    def layout_bytes(layout: tuple) -> int:
        """Size of a snapshot with these header sizes: (n_flat, n_rings, heads, window, embed_bytes, *flat, *ring rows)."""
        n_flat, n_rings, heads, window, embed_bytes = layout[:5]
        sizes = layout[5:]
        return SessionSnapshot.HEADER_BYTES + 16 + embed_bytes + sum(sizes[:n_flat]) + heads * window * sum(sizes[n_flat:])

    @property
    def device(self) -> torch.device:
        return self.data.device

    def to(self, device) -> "SessionSnapshot":
        """The snapshot in the memory of `device`: this object if it is there already, else a copy enqueued behind the event.
        From device memory or pinned host memory (what `cpu` and `load` return where a GPU is present) the copy is asynchronous;
        from pageable host memory it is staged and the host may wait for it."""
        dev = _cuda_device(device)
        if dev == self.data.device:
            return self
        if dev.type != "cuda":
            return self.cpu()
        data, ev = _copy_behind(self.data, self.event, dev)
        return SessionSnapshot(data, self.layout, ev)

    def cpu(self) -> "SessionSnapshot":
        """In host memory.  Waits for the kernel that fills the snapshot."""
        if not self.data.is_cuda:
            return self
        if self.event is not None:
            self.event.synchronize()
        return SessionSnapshot(self._pinned(self.data.cpu()), self.layout, None)

    @staticmethod
    def _pinned(host: torch.Tensor) -> torch.Tensor:
        """`host` in pinned memory where a GPU is present, so that a later `to(device)` does not stage the copy."""
        return host.pin_memory() if torch.cuda.is_available() else host

    def save(self, path: str):
        """The bytes of `data` as a file: the header makes it self-describing."""
        self.cpu().data.numpy().tofile(path)

    @classmethod
    def load(cls, path: str, device=None) -> "SessionSnapshot":
        """A snapshot from `save`'s file, in host memory or on `device`.  ValueError: not a snapshot, another layout version, or
        a size that does not match the header."""
        raw = np.fromfile(path, dtype=np.uint8)
        layout, total = cls._header(raw, path)
        if cls.layout_bytes(layout) != raw.size or total != raw.size:
            raise ValueError(f"{path}: {raw.size} bytes, the header's sizes make {cls.layout_bytes(layout)} (total word {total})")
        snap = cls(cls._pinned(torch.from_numpy(raw)), layout, None)
        return snap if device is None else snap.to(device)

    @classmethod
    def _header(cls, raw: np.ndarray, path: str):
        """(layout, total bytes) as the header at the start of `raw` states them.  ValueError: not a snapshot's header."""
        if raw.size < cls.HEADER_BYTES + 16:
            raise ValueError(f"{path}: {raw.size} bytes, not a session snapshot")
        head = raw[:cls.HEADER_BYTES].view("<u4").astype(np.int64)
        if head[0] != cls.MAGIC or head[1] != cls.VERSION:
            raise ValueError(f"{path}: magic {int(head[0]):#x} version {int(head[1])}, expected {cls.MAGIC:#x} version {cls.VERSION}")
        n_flat, n_rings = int(head[3]), int(head[4])
        if n_flat < 1 or n_rings < 1 or 8 + n_flat + n_rings > cls.HEADER_BYTES // 4:
            raise ValueError(f"{path}: header names {n_flat} state tensors and {n_rings} rings")
        return tuple(int(v) for v in head[3:8 + n_flat + n_rings]), int(head[2])


class SessionSnapshotBatch:
    """k listeners' snapshots as ONE value: what `SessionStreamer.suspend_many` / `drain` take out and `resume_many` puts back
    — a whole streamer moves in one launch and one copy.
    `data`: ONE uint8 tensor [k, stride]; row i holds snapshot i in its leading `nbytes` = `SessionSnapshot.layout_bytes(layout)`
    bytes (stride >= nbytes, a multiple of 16; what lies behind is padding nobody writes).  `layout` and `event` as for a
    `SessionSnapshot`: one layout, and ONE event behind the launch or copy that filled all of `data`.
    `batch[i]` is a `SessionSnapshot` whose `data` is a view of row i — same memory, same event — so `resume(slot, batch[i])`
    works, and `resume_many` recognises views of one batch and uses the batch in place.  `to` never waits for the device;
    `cpu`, `save` and `load` may."""

    def __init__(self, data: torch.Tensor, layout: tuple, event=None):
        self.data, self.layout, self.event = data, tuple(layout), event
        self.nbytes = SessionSnapshot.layout_bytes(self.layout)
        if data.dim() != 2 or data.dtype != torch.uint8 or data.stride(1) != 1 or data.shape[1] < self.nbytes or \
                data.shape[1] % 16 or (data.shape[0] > 1 and data.stride(0) != data.shape[1]):
            raise ValueError(f"a batch is a contiguous uint8 [k, stride >= {self.nbytes}, a multiple of 16], got "
                             f"{tuple(data.shape)} {data.dtype}")

    def __len__(self) -> int:
        return self.data.shape[0]

    def __getitem__(self, i: int) -> SessionSnapshot:
        i = range(len(self))[i]                             # negative indexes; IndexError ends an iteration
        snap = SessionSnapshot(self.data[i, :self.nbytes], self.layout, self.event)
        snap.batch, snap.index = self, i
        return snap

    @property
    def device(self) -> torch.device:
        return self.data.device

    def to(self, device) -> "SessionSnapshotBatch":
        """The batch in the memory of `device`: this object if it is there already, else ONE copy enqueued behind the event."""
        dev = _cuda_device(device)
        if dev == self.data.device:
            return self
        if dev.type != "cuda":
            return self.cpu()
        data, ev = _copy_behind(self.data, self.event, dev)
        return SessionSnapshotBatch(data, self.layout, ev)

    def cpu(self) -> "SessionSnapshotBatch":
        """In host memory.  Waits for the launch that fills the batch."""
        if not self.data.is_cuda:
            return self
        if self.event is not None:
            self.event.synchronize()
        return SessionSnapshotBatch(SessionSnapshot._pinned(self.data.cpu()), self.layout, None)

    @classmethod
    def stack(cls, snapshots, device=None) -> "SessionSnapshotBatch":
        """A batch of single snapshots of one layout, on `device` (default: where the first one lies).  One copy per snapshot,
        each ordered behind that snapshot's event on the device's current stream; the host does not wait for device memory."""
        snaps = list(snapshots)
        if not snaps:
            raise ValueError("no snapshots to stack")
        layout = snaps[0].layout
        for sn in snaps:
            if sn.layout != layout or sn.data.numel() != SessionSnapshot.layout_bytes(layout):
                raise ValueError(f"snapshots of different layouts: {sn.layout} ({sn.data.numel()} bytes) and {layout}")
        dev = _cuda_device(snaps[0].data.device if device is None else device)
        if dev.type != "cuda":
            return cls(SessionSnapshot._pinned(torch.stack([sn.cpu().data for sn in snaps])), layout, None)
        data = torch.empty(len(snaps), SessionSnapshot.layout_bytes(layout), dtype=torch.uint8, device=dev)
        cur = torch.cuda.current_stream(dev)
        for i, sn in enumerate(snaps):
            sn = sn.to(dev)
            if sn.event is not None:
                cur.wait_event(sn.event)
            sn.data.record_stream(cur)
            data[i].copy_(sn.data, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(cur)
        return cls(data, layout, ev)

    def save(self, path: str):
        """The k snapshots back to back, unpadded, each in `SessionSnapshot.save`'s format: a header's total word says where the
        next one starts."""
        self.cpu().data[:, :self.nbytes].contiguous().numpy().tofile(path)

    @classmethod
    def load(cls, path: str, device=None) -> "SessionSnapshotBatch":
        """A batch from `save`'s file, in host memory or on `device`.  ValueError: not snapshots back to back, sizes that do not
        add up, or snapshots of more than one layout."""
        raw = np.fromfile(path, dtype=np.uint8)
        layout, total = SessionSnapshot._header(raw, path)
        n = SessionSnapshot.layout_bytes(layout)
        if total != n or raw.size % n:
            raise ValueError(f"{path}: {raw.size} bytes, the first header's sizes make {n} (total word {total})")
        rows = raw.reshape(-1, n)
        for i in range(1, rows.shape[0]):
            if SessionSnapshot._header(rows[i], path) != (layout, total):
                raise ValueError(f"{path}: snapshot {i} has another layout than snapshot 0")
        batch = cls(SessionSnapshot._pinned(torch.from_numpy(rows)), layout, None)
        return batch if device is None else batch.to(device)


class SessionStreamer:
    """A batched `Streamer` whose rows are listener SLOTS that open, close and fail one at a time.

    The chunk loop stays what `Streamer` runs — same buffers, same launches, all slots advance together, one chunk per
    `step` — between two more graph nodes (include/lookonce_hip.h, "streaming sessions"): `lh_session_begin` zeroes the
    state of a slot that was just opened or closed and hands only live slots' samples to the separator; `lh_session_end`
    silences idle slots and closes a slot whose chunk was, or came out, non-finite.  A fault therefore costs ONE listener
    their session: `step` never raises for it, the other rows keep their bits, and the slot can be opened again at once.
      * `open(slot, embed)`: from the next `step` on the slot is a fresh stream (zero tails, (h, c) and K / V history — the
        zero history is the same in every rotation of the ring, so the shared ring position needs no per-slot copy) with
        its own speaker gain;  `close(slot)`: from the next `step` on its output rows are exact zeros;
      * `set_embedding(slot, embed)` re-targets an open slot, its carried state is kept;
      * `faults()`: slots the device closed since they were opened;  `active`: the open slots that have not faulted.
    Nothing here waits for the device: commands travel as one asynchronous copy of a pinned array ahead of the replay
    (only when something is pending), the fault words are pinned host memory the last kernel stores to.
    Enrollment (`enroll_chunks` = n >= 2; 0, the default, builds exactly the object above): "look once" from the listener's
    own stream.  `enroll(slot, embedder)` arms an idle slot: one more graph node (`lh_session_capture`, after
    `lh_session_begin`) records the slot's next n chunks — the 128 n contiguous samples from the next `step` on — into a
    device buffer and posts a word in pinned host memory when the clip is complete.  `poll()` (the first thing `step` does;
    public, cheap, idempotent) reads those words: the clips completed since the last poll go through ONE `embedder` call, a
    batch in ascending slot order, on the streamer's one side stream behind an event of the loop's stream; a call whose
    second event reports complete hands its rows to the `open` path, and the slot is in `active` and a fresh stream from that
    `step` on.  `enrolling`: the slots capturing or embedding;  `embedding_of(slot)`: the [256] device tensor enrollment
    opened the slot with (keep it to `open` the listener again later).  Meanwhile the slot is idle to the separator: its
    output rows are exact zeros — or their own input, with `passthrough=True` in a monitor streamer (below).  An inf / NaN among
    the recorded samples aborts the capture: the slot is listed by `faults()` and is idle again, to be enrolled or opened at
    once.  `close(slot)` cancels a capture or a running embedding (a result that arrives later is dropped by its
    generation), `reset()` cancels all of them.  Call the embedder once on a clip of this length before the loop starts:
    its first call packs weights.
    Compaction (`compact=True`; False, the default, builds exactly the object above): a chunk costs what its listeners cost.
    Slots keep their numbers towards the caller — every method above, the rows of `step`'s input and output, the fault
    words — while the open listeners live in the leading ROWS of the same state buffers, and `step` runs the chunk's kernels
    for `last_rows` = the smallest of `row_buckets` that holds the `rows_in_use` rows (one alternating graph pair per
    bucket, over the leading rows of the same buffers and workspace).  An opening takes the first free row.  When a
    listener leaves — `close`, or a fault word `step` sees — the survivors in the rows at and above the new row count move
    into the holes below it, highest row first: every move has src >= the new count > dst, so the moves of one step are
    disjoint and run in one launch (`lh_session_move`, the chunk's first node: the row's slice of every state tensor, its
    speaker gain, its `active` and pending device command word — bytes, the listener keeps their bits).  An opening of the
    same step takes the uppermost of the holes, which saves that move.  `lh_session_begin_rows` / `lh_session_end_rows` gather
    the row's input from, and scatter its output to, the slot; rows without a listener are idle on the device whatever they
    still hold, and a slot without a row is written zeros in every chunk.  Moves, the row <-> slot maps and the commands travel
    in the one asynchronous copy, only when something is pending.  A slot that is capturing or embedding owns no row.
    Pacing (`pace=True`; False, the default, builds exactly the object above, launch for launch): listeners do not arrive in
    lock-step.  `step(chunks, present)` HOLDS every slot whose `present[s]` is false: its input row is ignored (it may be NaN
    and is never judged for a fault), its output row is exact zeros, and every bit of its carried state — tails, (h, c), K / V
    rings and ring position — is after the step what it was before.  A listener's output stream is the concatenation of the
    output rows of the steps they were present for.  Every ROW owns its ring position: the chunk that serves an OPEN sets it
    to 0 and only a chunk the row consumed advances it (`lh_qkv_proj_ln_rows`, `lh_ring_advance_rows`), so in a paced streamer
    a listener's bits depend on their own chunks only — not on when they were opened, not on who else was held.  Commands are
    served whether or not the slot is held: a slot opened and held in the same step is reset and active, and its first chunk
    is the first one it is present for; a capturing slot that is held records nothing, its clip is the samples of the chunks
    it was present for.  With `compact=True` the position word moves with the row, and the hold words stay addressed by slot.
    The hold words travel like the commands, a fresh pinned array copied asynchronously, and only in a step whose mask differs
    from the one on the device: a steady all-present loop copies nothing.  A held row costs what a live row costs — its
    kernels run on a zero-gated input and `lh_session_end_paced` puts the row's state back, about 0.2 MB of copies — so
    pacing buys correctness under jitter, not time; a compacting streamer does not skip held rows.
    Suspend / resume (every flavour above, as source and as target, in any combination): `suspend(slot)` takes an open
    listener's state, as of the last `step`, out as a `SessionSnapshot` — one launch (`lh_session_save`) into a fresh device
    tensor: the tails and (h, c) of the ping-pong set the next chunk would read, the 50 window rows per head of every ring, the
    ring position (the row's own, or the shared counter), the speaker embedding and the row's two device words — and closes the
    slot.  `resume(slot, snapshot)` makes an idle slot that listener again from the next `step` on: `step` enqueues
    `lh_session_restore` behind its copy of the command words and ahead of the chunk (eager launches between two replays,
    like `set_embedding`'s; the graphs are what they were), and the slot opens WITHOUT a reset.  Into a paced streamer the ring
    rows and the position go back as they were, and the listener's output continues bit for bit; into a lock-step streamer the
    ring rows are rotated so that the listener's oldest row is the next one the shared counter overwrites — bit for bit when
    the shared position equals the saved one, within the tolerance of a listener opened at an arbitrary position otherwise.
    A compacting streamer plans a resume as an opening: it takes a hole, which no move of that step reads or writes; a slot
    closed or suspended and resumed between two steps gives its previous listener's row up first, like any listener that left.  A
    listener the device had closed in the chunk before `suspend` (the fault word not yet seen) makes a dead snapshot: resuming
    it leaves the slot idle on the device and lists it in `faults()` after that `step`.  Neither call waits for the device.
    Many at once: `suspend_many(slots)` / `drain()` / `resume_many(slots, snapshots)` are those calls in order for any number of
    listeners with a number of launches that does not depend on it — one `lh_session_save_rows` into one `SessionSnapshotBatch`
    tensor; in `step` one `lh_session_restore_rows` and one `lh_embed_proj_ln_rows` per batch, behind one copy of an item table.
    `suspend`, `resume` and a streamer that never calls the batched methods enqueue what they always did.
    Packets (`pace=True, packets=True`; False, the default, builds exactly the object above, launch for launch): clients do not
    send windows, they send contiguous PCM in packets of 10 or 20 ms that arrive with jitter.  `push({slot: samples [2, n]})`
    takes one tick's packets at any size — one fresh pinned buffer (an item table, then the samples), one asynchronous copy,
    one launch (`lh_session_feed`) that scatters them into a device FIFO of `fifo_samples` per slot — and `step()` takes no
    input: the chunk's first node (`lh_session_frame`) cuts a 192-sample window for every slot that holds one, writes the hold
    words of the others itself, and everything behind `chunk_in` and `hold` is the paced streamer.  The FIFO's two sample
    counters per slot wrap modulo 2^32 and are mirrored on the host in the same arithmetic: the host knows what every launch
    will find (`buffered(slot)`, `ready()`, `last_present` — a tuple of S bools, the slots the last `step` consumed a chunk
    of), the device follows, nothing is read back and no hold word travels.  A listener's output is the concatenation of
    their rows over the steps with `last_present[slot]`, whatever the packet sizes were; a slot with two chunks buffered is
    stepped twice (`while ss.ready(): ss.step()` catches up), a slot without one is held.  `push` raises `BufferError`, before
    anything is enqueued for any slot, when a slot would hold more than `fifo_samples`: the device FIFO cannot overflow.
    `flush(slot)` drops a slot's buffered input (with its next packet, or in a push of its own that `step` issues); `reset()`
    flushes everyone.  The FIFO is transport, not listener state: `open`, `close`, `enroll`, `suspend` and `resume` do not touch
    it and it is in no snapshot — a host that gives a slot to another client flushes it.  An idle slot is framed like any
    other, as lock-step gates an idle slot's row.  The last chunk of a stream needs its 64 look-ahead samples: push 64 zeros
    for the tail.  `pcm16=True`: packets are int16 (scaled by 2^-15 on the device, exact) and `step` returns int16 rows
    (`lh_session_emit_s16`, round half even, saturating) — the bits of the fp32 path fed `pcm.float() / 32768`.
    Client rate (`packets=True, client_rate=48000`; 16000, the default, builds exactly the object above, launch for launch):
    headsets and WebRTC stacks capture and play at 48 kHz, some at 32, 24 or 8.  `push` takes `[2, n]` at the client's rate and
    `step()` returns `[S, 2, hop_client]`, `hop_client = 128 * client_rate / 16000` samples at that rate (fp32, or int16 with
    `pcm16`) — resampled on the device with the arithmetic of `resample.Resampler` (torchaudio's `sinc_interp_hann`, one fp32
    inner product that every kernel shares): the packets land through `lh_session_feed` in a second per-slot ring at the client
    rate, `lh_session_resample_in` (one more launch of the same `push`, its items in the same copy) turns whole blocks of it into
    16 kHz samples of the FIFO, and `lh_session_resample_out`, the chunk's last node, turns the 16 kHz rows into client rows.
    What a listener hears equals `Resampler(client_rate, 16000)` of their whole stream, served by a 16 kHz packet streamer, then
    `Resampler(16000, client_rate)` of `delay_out` zeros followed by the rows — bit for bit, whatever the packet sizes.  Rates
    are multiples of 125 Hz (a chunk is then a whole number of client samples): 8000, 24000, 32000, 40000, 48000, 96000 ...;
    44100 needs `any_rate=True` (below) and is refused without it.  `fifo_samples`, `buffered`, `ready`, `last_present` and
    `BufferError` keep their meaning in 16 kHz samples: the host mirrors the resampler's block arithmetic in integers.
    Added latency: a 16 kHz block is made when its `lookahead_in = width + o - 1` later client samples have been pushed (48 kHz:
    21 samples, 0.44 ms), and the output is `delay_out` 16 kHz samples late (toward 48 kHz: 8 samples, 0.5 ms); the tail of a
    stream needs `lookahead_in` zeros pushed behind it (and the 64 look-ahead samples of the last chunk, at the client's rate).
    The raw ring and the output tail are transport like the FIFO: in no snapshot, untouched by `open`, `close`, `suspend` and
    `resume`; `flush(slot)` and `reset()` clear them, so a flushed slot's stream starts from silence, as torchaudio's left pad
    does.  Enrollment keeps recording the 16 kHz `chunk_in`.
    Any rate (`client_rate=44100, any_rate=True`; False, the default, and any multiple of 125 Hz with it build exactly the object
    above, launch for launch): consumer capture and playback run at 44.1 kHz, where a chunk is 352.8 client samples.  The hop is
    FRACTIONAL: `step()` returns `[S, 2, hop_client]` with `hop_client = ceil(128 client_rate / 16000)` (353), and
    `last_counts[slot]` — host arithmetic, nothing is read back — says how many leading samples of the slot's row are the next
    ones of its stream: 352, 353, 353, 353, 353 over a period of 5 live steps, 0 for a held slot (every packet streamer has
    `last_counts`: `hop_client`, or 128, for a present slot elsewhere); the columns behind are zeros.  The last node is
    `lh_session_resample_out_any` (include/lookonce_hip.h, "any rate": the slot's phase in the period is a device word, mirrored
    here), the input side is the one above.  What a listener hears is the same chain, bit for bit, with `delay_out = width + o
    - 1` 16 kHz samples — 166, 10.4 ms toward 44.1 kHz — on the way out and `lookahead_in` = 457 client samples (10.4 ms) on the
    way in: about 21 ms in all, the price of keeping torchaudio's block arithmetic to the bit.  The phase is transport like the
    tail: in no snapshot, zeroed by `flush(slot)` and `reset()` only.  22050, 11025 and 88200 Hz are served alike; a rate that
    would carry more per slot than 11025 Hz does is refused at construction.
    Monitor (`monitor=True`; False, the default, builds exactly the object above, launch for launch): what a listener hears is
    `wet` x their separated rows + `dry` x their own input.  `set_mix(slot, wet, dry)` (finite, in [0, 1]; any slot, idle ones
    included) holds from the next `step`, `mix_of(slot)` returns the targets.  One more graph node after the end node and ahead of
    the resample / 16-bit node (`lh_session_mix`, by slot in every flavour) ramps the slot's two gains towards the targets on the
    device — linear, `monitor_ramp` 16 kHz samples per full swing, exactly on target at the end, re-targetable in mid-ramp — and
    mixes in place: output row j covers samples [128 j, 128 j + 128) of the slot's stream, the first 128 samples of input row j, so
    the dry path needs no delay line and is aligned to the sample behind any framing and resampling.  A slot settled at the
    defaults (1, 0) keeps the bits of a streamer without the node; a held slot's row stays zeros and its ramp waits; a non-finite
    sample among the row's own 128 silences that row without a fault.  The targets travel like the hold words (a fresh pinned
    array, one asynchronous copy, only in a step where one changed).  The mix is transport, like the FIFO: in no snapshot,
    untouched by `open`, `close`, `suspend`, `resume` and row moves; `reset()` puts it back to (1, 0).  `enroll(slot, embedder,
    passthrough=True)` posts (0, 1) with the arming and (1, 0) in the step that opens the slot: the room, then a click-free
    cross-fade into the target from the slot's first live chunk.  A slot the device closed for a fault is idle and sounds as an
    idle slot with its dry gain sounds: fail-open.
    Re-look (`relook(slot, embedder)`; needs `enroll_chunks`, not `monitor`): the capture runs on an OPEN slot while the separator
    goes on with the current embedding — the slot is in `active` and in `enrolling`, keeps its row in a compacting streamer, and
    its output is bit for bit what it would be without the capture — and the finished embedding takes the `set_embedding` path:
    state kept, `embedding_of(slot)` updated.  `close` cancels the look and closes the session, `suspend` is refused meanwhile.
        ss = net.make_session_streamer(64, "cuda:0", pace=True, packets=True)
        ss.open(0, emb_a); ss.open(1, emb_b)
        while serving:                                       # one tick: whatever arrived, then the chunks that are ready
            ss.push({0: a.recv(160), 1: b.recv(320)})        # a 10 ms and a 20 ms client, [2, n] float32 each
            while ss.ready():
                y = ss.step()
                for slot, took in enumerate(ss.last_present):
                    if took:
                        send(slot, y[slot])                  # [2, 128], the next 8 ms of that listener
    A snapshot is only meaningful under the weights it was taken with: that is the caller's to keep."""
    RESET, OPEN, CLOSE, GEN_SHIFT, MAX_SPANS, GEN_MASK = 1, 2, 4, 8, 32, 0x7fffff      # LH_SESSION_*
    ARM, CANCEL, ENROLL_FAULT = 1, 2, 0x80000000                                       # LH_ENROLL_*
    FEED_F32, FEED_S16, FEED_FLUSH, FEED_ITEM_WORDS = 0, 1, 1, 5                       # LH_FEED_*, lh_feed_item_t
    HOP, WINDOW, COUNTER_MASK = 128, 192, 0xffffffff                                   # samples a chunk consumes / needs
    RATE, RESAMPLE_ITEM_WORDS = 16000, 4                                               # the model's rate; lh_resample_item_t
    MAX_RATIO, ANY_RATE_STAGE = 4096, 1427                                             # RS_MAX_RATIO; RA_XS of lh_stream.hip

    def __init__(self, net: Net, n_slots: int, device, use_graph: bool = True, enroll_chunks: int = 0, compact: bool = False,
                 row_buckets=None, pace: bool = False, packets: bool = False, fifo_samples: int = 2048, pcm16: bool = False,
                 client_rate: int = 16000, monitor: bool = False, monitor_ramp: int = 256, any_rate: bool = False):
        if n_slots < 1:
            raise ValueError("n_slots must be positive")
        if client_rate != self.RATE:
            if not packets:
                raise ValueError("client_rate is the sample rate of a packet streamer's clients: packets=True")
            if int(client_rate) != client_rate or not 1000 <= client_rate <= 384000 or (client_rate % 125 and not any_rate):
                raise ValueError(f"client_rate must be a multiple of 125 Hz in [1000, 384000] — a 128-sample chunk at 16 kHz is "
                                 f"then a whole number of client samples (8000, 24000, 32000, 48000 ...); {client_rate} is not "
                                 "(44100 is not either): any_rate=True serves such a rate with a fractional hop")
            if client_rate % 125 and max(self.RATE, client_rate) // math.gcd(self.RATE, client_rate) > self.MAX_RATIO:
                raise ValueError(f"client_rate {client_rate}: 16000 / {client_rate} in lowest terms has a term above "
                                 f"{self.MAX_RATIO}, more than the resampling kernels take")
        if packets and not pace:
            raise ValueError("packets are the input of a paced streamer (the device decides who is present): pace=True")
        if pcm16 and not packets:
            raise ValueError("pcm16 is the sample format of a packet streamer: packets=True")
        if packets and (fifo_samples < 256 or fifo_samples & (fifo_samples - 1) or fifo_samples > 1 << 24):
            raise ValueError(f"fifo_samples must be a power of two in [256, 2^24] (a 192-sample window while 128 more "
                             f"arrive; the ring index is a mask), got {fifo_samples}")
        if row_buckets is not None and not compact:
            raise ValueError("row_buckets are the launch sizes of a compacting streamer: compact=True")
        if compact:
            if row_buckets is None:
                row_buckets = [1 << i for i in range(n_slots.bit_length()) if 1 << i < n_slots] + [n_slots]
            row_buckets = tuple(int(b) for b in row_buckets)
            if not row_buckets or row_buckets[0] < 1 or row_buckets[-1] != n_slots or \
                    any(a >= b for a, b in zip(row_buckets, row_buckets[1:])):
                raise ValueError(f"row_buckets must ascend from >= 1 to n_slots = {n_slots}, got {row_buckets}")
        if isinstance(monitor_ramp, bool) or not isinstance(monitor_ramp, int) or monitor_ramp < 1:
            raise ValueError(f"monitor_ramp is the number of 16 kHz samples of a full 0 -> 1 swing, an int >= 1, got "
                             f"{monitor_ramp!r}")
        if enroll_chunks < 0 or enroll_chunks == 1:
            raise ValueError("enroll_chunks must be 0 (no enrollment) or >= 2: the embedder needs 4 STFT frames at stride 64, "
                             "192 samples, and a chunk records 128")
        # buffers, packed weights, workspace and staleness checks are a Streamer's; its graphs are not captured
        self._st = st = Streamer(net, n_slots, device, use_graph=False)
        self.net, self.S, self.device = net, n_slots, st.device
        S, dev = n_slots, st.device
        self.chunk_in = torch.zeros_like(st.chunk)          # as the clients sent it; `st.chunk` is the gated copy
        self.out = st.out
        self.compact, self.row_buckets = bool(compact), row_buckets
        if compact:
            # rows of words: move table | row -> slot | slot -> row | cmd from the host || cmd from the device | active.
            # The first four are the host's (one copy), the last three the [2][S] cmd and the [S] active of the kernels
            self.out = torch.zeros_like(st.out)             # by SLOT; `st.out` is by row
            self._tables = torch.zeros(6, S, dtype=torch.int32, device=dev)
            self._tables[1:3].fill_(-1)
            self._words = self._tables[3:]
        else:
            self._words = torch.zeros(3, S, dtype=torch.int32, device=dev)   # cmd from the host | cmd from the device | active
        self._fault = net._host_words(S, dev)
        self._fault_np = self._fault.numpy()                # the same memory, read without a tensor op per slot
        table = lambda ts: (_Span * len(ts))(*[_Span(t.data_ptr(), t.numel() * t.element_size() // S) for t in ts])
        carried, rings = [st._carried(0), st._carried(1)], [t for kv in st.rings for t in kv]
        state = carried[0] + carried[1] + rings
        if len(state) + compact > self.MAX_SPANS:
            raise ValueError(f"{len(state) + compact} state tensors, lh_session_begin / lh_session_move take {self.MAX_SPANS}")
        self._spans = table(state)
        if compact:                                         # what a row owns: its state and its speaker gain
            self._spans_move = table(state + [st.gain])
        # what chunk k WRITES: the (h, c) of the other ping-pong set
        self._spans_end = [table(st.sets[k ^ 1]["h"] + st.sets[k ^ 1]["c"]) for k in (0, 1)]
        # suspend / resume: the tails and (h, c) of each ping-pong set, the rings with their geometry, the snapshot's sizes
        self._spans_live = [table(c) for c in carried]
        self._spans_rings = (_Span * len(rings))(*[_Span(t.data_ptr(), t.shape[-1] * t.element_size()) for t in rings])
        self._ring_geom = (net.n_head, rings[0].shape[1], net.local_atten_len)      # heads per slot, rows per head, window
        self._snap_layout = (len(self._spans_live[0]), len(rings), net.n_head, net.local_atten_len,
                             st.embed.shape[1] * st.embed.element_size(), *[sp.bytes for sp in self._spans_live[0]],
                             *[sp.bytes for sp in self._spans_rings])
        self._snap_bytes = SessionSnapshot.layout_bytes(self._snap_layout)
        self.pace = bool(pace)
        if pace:
            self._ring = torch.zeros(2, S, dtype=torch.int32, device=dev)    # per row: ring position | the chunk's write slot
            self._hold = torch.zeros(S, dtype=torch.int32, device=dev)       # per slot, as of the last copy: `_held`
            self._none_held = (False,) * S
            # what a held row gets back: (read, written) of every tail and (h, c), for chunk k
            pairs = [[t for rw in zip(carried[k], carried[k ^ 1]) for t in rw] for k in (0, 1)]
            if len(pairs[0]) > self.MAX_SPANS:
                raise ValueError(f"{len(pairs[0]) // 2} state pairs, lh_session_end_paced takes {self.MAX_SPANS // 2}")
            self._spans_carry = [table(p) for p in pairs]
        self.packets, self.pcm16, self.fifo_samples = bool(packets), bool(pcm16), int(fifo_samples)
        if packets:
            R = self.fifo_samples
            self._fifo = torch.zeros(S, net.num_ch, R, device=dev)           # a ring per slot and channel
            self._fifo_words = torch.zeros(2, S, dtype=torch.int32, device=dev)      # wr | rd: sample counters mod 2^32
            # one tick's item table and samples: at most a full ring per slot (`push` refuses more)
            self._item_words = (self.FEED_ITEM_WORDS * S + 3) // 4 * 4
            self._stage = torch.zeros(self._item_words + S * net.num_ch * R // (2 if pcm16 else 1), dtype=torch.int32, device=dev)
            if pcm16 and client_rate == self.RATE:
                self.out16 = torch.zeros(S, net.n_srcs, net.stft_chunk_size, dtype=torch.int16, device=dev)
        self.client_rate, self.hop_client, self._resampling = int(client_rate), self.HOP, client_rate != self.RATE
        self._fractional = self._resampling and client_rate % 125 != 0      # `any_rate`: a chunk is no whole number of samples
        if self._resampling:
            from .resample import resample_bank
            bank_in, self._w_in, self._o_in, self._n_in = resample_bank(self.client_rate, self.RATE)
            bank_out, self._w_out, self._o_out, self._n_out = resample_bank(self.RATE, self.client_rate)
            self._k_in = 2 * self._w_in + self._o_in
            self.hop_client = self.HOP * self._o_in // self._n_in
            self.lookahead_in = self._w_in + self._o_in - 1                  # client samples behind a block's first one
            self.delay_out = (self._w_out + 2 * self._o_out - 1) // self._o_out * self._o_out       # 16 kHz samples, D o
            tail = self._w_out + self.delay_out
            if self._fractional:                            # lh_session_resample_out_any: d, P, T and hop_max of the header
                o, n = self._o_out, self._n_out
                self.hop_client = -(-self.HOP * n // o)
                self.delay_out = self._w_out + o - 1
                self._period = o // math.gcd(self.HOP, o)
                tail = 2 * self._w_out + 2 * o + -(-o // n) - 1
                if tail + self.HOP > self.ANY_RATE_STAGE:
                    raise ValueError(f"client_rate {client_rate}: 16000 / {client_rate} = {o} / {n} carries {tail} samples per "
                                     f"slot and channel; the resample node stages {self.ANY_RATE_STAGE - self.HOP}, what 11025 Hz "
                                     "needs")
                bank_out = bank_out.t().contiguous()        # [K][n]: a wave's consecutive phases read consecutive floats
            # a full FIFO's worth of input plus one block's taps: what `push` can leave unconsumed
            self.raw_samples = 256
            while self.raw_samples < self.fifo_samples * self._o_in // self._n_in + self._k_in:
                self.raw_samples *= 2
            Rin = self.raw_samples
            self._raw = torch.zeros(S, net.num_ch, Rin, device=dev)          # a ring per slot and channel, at the client rate
            self._raw_words = torch.zeros(2, S, dtype=torch.int32, device=dev)       # its wr | rd (rd: only FLUSH writes it)
            self._tap0 = -self._w_in & self.COUNTER_MASK                     # a stream's first tap: the left pad lies below 0
            self._tail = torch.zeros(S, net.n_srcs, tail, device=dev)
            if self._fractional:                            # the device's phase and count words; the host mirrors both
                self._phase, self._count = torch.zeros(2, S, dtype=torch.int32, device=dev)
            self.out_client = torch.zeros(S, net.n_srcs, self.hop_client, dtype=torch.int16 if pcm16 else torch.float32,
                                          device=dev)
            self._bank_in, self._bank_out = bank_in.to(dev), bank_out.to(dev)
            self._ritem_off = self.FEED_ITEM_WORDS * S                       # the resample items follow the feed items
            self._item_words = ((self.FEED_ITEM_WORDS + self.RESAMPLE_ITEM_WORDS) * S + 3) // 4 * 4
            self._stage = torch.zeros(self._item_words + S * net.num_ch * Rin // (2 if pcm16 else 1), dtype=torch.int32, device=dev)
        self._next_gen = 1                                  # generations outlive `reset`: a late embedding is told by its own
        self._jobs = []                                     # embedder calls in flight, oldest first: (event, slots, gens, out)
        self.enroll_chunks = n = enroll_chunks
        self.monitor, self.monitor_ramp = bool(monitor), monitor_ramp
        if monitor:
            self._mix = torch.zeros(2, 2, S, device=dev)    # targets [2][S] | gains [2][S]: wet, then dry
            self._mix[:, 0].fill_(1.0)
            self._mix_step = float(np.float32(1.0) / np.float32(monitor_ramp))
        if n:
            self._clips = torch.zeros(S, net.num_ch, net.stft_chunk_size * n, device=dev)
            self._ewords = torch.zeros(3, S, dtype=torch.int32, device=dev)      # ecmd | estate: generation, chunks recorded
            self._edone = net._host_words(S, dev)
            self._edone_np = self._edone.numpy()
            self._side = net._enroll_side(dev)
        self._reset_host()
        self.graphs = None
        if use_graph:
            with torch.no_grad():
                if compact:                                 # one alternating pair per launch size
                    self.graphs = {n: Streamer._capture(lambda k, n=n: self._body(k, n), dev) for n in row_buckets}
                else:
                    self.graphs = Streamer._capture(self._body, dev)
            self.reset()

    def _body(self, k: int, n_rows: int = 0):
        """The chunk that reads ping-pong set k: (frame ->) (move ->) begin -> (capture) -> the separator's chunk -> ring advance
        -> end (-> mix) (-> resample out | 16-bit out), every node in the form of this streamer.  The `_rows` forms of a
        compacting one serve its leading `n_rows` rows — every per-row tensor is row-major in the batch index, so the leading
        rows of the same buffers are a batch of n — and take the row <-> slot maps; the `_paced` forms take the hold words and
        every row's own ring position and write slot.  Without compaction every slot is a row, whatever `n_rows` says."""
        st, net, S = self._st, self.net, self.S
        P, A = (lambda t: t.data_ptr()), ctypes.addressof
        with net._device_ctx(st.chunk):
            lib, stream = net._lib(st.chunk), net._stream(self.device)
            rows, paced = "_rows" * self.compact, "_paced" * self.pace
            x, spans, end, cmd, active = P(self.chunk_in), self._spans, self._spans_end[k], P(self._words), P(self._words[2])
            n, chunk = (n_rows, st.chunk[:n_rows]) if self.compact else (S, st.chunk)
            # what only the `_rows` forms take, then what only the `_paced` forms take: empty for the others
            count = (n, S) if self.compact else (S,)
            frm, slot_of, row_of = ((P(t),) for t in self._tables[:3]) if self.compact else ((), (), ())
            out = (P(self.out),) if self.compact else ()    # by slot; `st.out` is by row
            hold = (P(self._hold),) if self.pace else ()
            pos = (P(self._ring[0]), P(self._ring[1])) if self.pace else ()
            carry = (A(self._spans_carry[k]), len(self._spans_carry[k]) // 2) if self.pace else ()
            if self.packets:                                # the windows and the hold words of this chunk, made on the device
                lib.call("lh_session_frame", P(self._fifo), P(self._fifo_words[0]), P(self._fifo_words[1]), x, *hold,
                         self.fifo_samples, S, stream)
            if self.compact:
                move = self._spans_move
                lib.call("lh_session_move" + paced, A(move), len(move), *frm, cmd, active, *pos[:1], n, S, stream)
            lib.call("lh_session_begin" + rows + paced, A(spans), len(spans), x, P(st.chunk), cmd, active, *slot_of, *hold, *pos,
                     *count, stream)
            if self.enroll_chunks:                          # by slot, like the hold words: a capturing slot owns no row
                lib.call("lh_session_capture" + paced, x, P(self._clips), P(self._ewords), P(self._ewords[1]), P(self._edone),
                         *hold, self.enroll_chunks, S, stream)
            net._stream_chunk(chunk, st.gain, st.sets[k], st.sets[k ^ 1], st.rings, st.pos, st.out, st._pk, st._ws, None,
                              keep_nonfinite=1, write_pos=self._ring[1] if self.pace else None)
            if self.pace:
                lib.call("lh_ring_advance_rows", *pos, net.local_atten_len, n, stream)
            else:
                lib.call("lh_ring_advance", P(st.pos), net.local_atten_len, stream)
            lib.call("lh_session_end" + rows + paced, A(end), len(end), *carry, x, P(st.out), *out, cmd, active, P(self._fault),
                     *hold, *slot_of, *row_of, *frm, *count, stream)
            if self.monitor:                                # by slot in every flavour, on the rows the end node left
                lib.call("lh_session_mix", x, P(self.out), P(self._mix[0]), P(self._mix[1]), *(hold or (None,)), self._mix_step,
                         S, stream)
            if self._fractional:                            # a fractional hop at the client's rate, counted on the device
                lib.call("lh_session_resample_out_any", P(self.out), P(self._tail), P(self._phase), *hold, P(self.out_client),
                         P(self._count), self.FEED_S16 if self.pcm16 else self.FEED_F32, S, P(self._bank_out), self._o_out,
                         self._n_out, self._w_out, stream)
            elif self._resampling:                          # the rows at the client's rate, fp32 or 16-bit
                lib.call("lh_session_resample_out", P(self.out), P(self._tail), *hold, P(self.out_client),
                         self.FEED_S16 if self.pcm16 else self.FEED_F32, S, P(self._bank_out), self._o_out, self._n_out,
                         self._w_out, stream)
            elif self.pcm16:
                lib.call("lh_session_emit_s16", P(self.out), P(self.out16), S, stream)

    def _reset_host(self):
        """The host's mirrors of the device words, and what is pending for the next `step`: as in a new SessionStreamer."""
        S = self.S
        self._gen = [0] * S                                 # generation of the slot's current opening, 0 = idle
        self._pending = {}                                  # slot -> command word for the next step
        self._resumes = {}                                  # slot -> [snapshot, embedding set since `resume` or None]
        self._resume_batches = []                           # `resume_many`: (batch, {slot: (index, the slot's entry above)})
        self._capturing = {}                                # slot -> (generation, embedder) of a capture in progress
        self._embedding = {}                                # slot -> generation of a clip the embedder is running on
        self._enroll_faults = set()                         # idle slots whose last capture the device aborted
        self._enrolled = {}                                 # slot -> the embedding enrollment opened it with
        self._epending = {}                                 # slot -> LH_ENROLL_* word for the next step
        self._relook = set()                                # capturing / embedding slots whose session stays open: `relook`
        self._passthrough = set()                           # enrolling slots whose mix goes back to (1, 0) with their OPEN
        if self.compact:
            self._row_of, self._slot_of = [-1] * S, [-1] * S                 # as of the last `step`
            self._n_rows = 0
            self._last_rows = self.row_buckets[0]
            # slot and generation of the listener in each row: one vector compare per `step` finds a fault word
            self._slot_np, self._rgen_np = np.zeros(S, dtype=np.int64), np.full(S, -1, dtype=np.int64)
        if self.pace:
            self._held = self._none_held                    # the hold words as of the last copy
        if self.packets:
            self._wr, self._rd = [0] * S, [0] * S           # the FIFO's two counters: the device follows
            self._flush = set()                             # slots whose next item carries FLUSH
            self.last_present = (False,) * S
        if self._resampling:
            self._raw_wr, self._tap = [0] * S, [self._tap0] * S              # raw samples pushed | next block's first tap
        if self._fractional:
            self._phase_of, self._last_counts = [0] * S, (0,) * S            # live steps taken mod P | the last step's counts
        if self.monitor:
            self._targets = [(1.0, 0.0)] * S                # the host's copy of the targets, as fp32 values
            self._mix_posted = True                         # false: a target changed since the last copy

    def reset(self):
        """Every slot idle, all state zero (what a new SessionStreamer starts from).  Captures and embeddings are cancelled:
        calls in flight finish, their rows are dropped by generation."""
        self._st.reset()
        if self.pace:
            self._ring.zero_()
            self._hold.zero_()
        if self.packets:                                    # every slot flushed
            self._fifo_words.zero_()
        if self._resampling:
            for t in (self._raw, self._raw_words, self._tail, self.out_client):
                t.zero_()
        if self._fractional:
            self._phase.zero_()
            self._count.zero_()
        if self.compact:
            self._tables.zero_()
            self._tables[1:3].fill_(-1)
            self.out.zero_()
        self._words.zero_()
        self._fault.zero_()
        if self.enroll_chunks:
            self._ewords.zero_()
            self._edone.zero_()
        if self.monitor:                                    # gains and targets: wet 1, dry 0
            self._mix.zero_()
            self._mix[:, 0].fill_(1.0)
        self._reset_host()

    def set_mix(self, slot: int, wet: float, dry: float):
        """From the next `step` on `slot` sounds `wet` x its separated rows + `dry` x its own input samples (a monitor
        streamer: `monitor=True`), each gain ramped on the device from where it stands, `monitor_ramp` samples per full
        swing.  Any slot, idle ones included: an idle slot's separated rows are zeros, so it sounds `dry` x the room."""
        self._slot(slot)
        if not self.monitor:
            raise ValueError("this SessionStreamer was built without a monitor: make_session_streamer(..., monitor=True)")
        wet, dry = float(wet), float(dry)
        if not (math.isfinite(wet) and math.isfinite(dry) and 0.0 <= wet <= 1.0 and 0.0 <= dry <= 1.0):
            raise ValueError(f"wet and dry are finite gains in [0, 1], got ({wet}, {dry})")
        target = (float(np.float32(wet)), float(np.float32(dry)))
        if target != self._targets[slot]:
            self._targets[slot] = target
            self._mix_posted = False

    def mix_of(self, slot: int) -> tuple:
        """(wet, dry): the targets of `slot`'s mix, as the device gets them (fp32 values)."""
        self._slot(slot)
        if not self.monitor:
            raise ValueError("this SessionStreamer was built without a monitor: make_session_streamer(..., monitor=True)")
        return self._targets[slot]

    def _slot(self, slot: int) -> int:
        if not 0 <= slot < self.S:
            raise IndexError(f"slot {slot} out of range for {self.S} slots")
        return slot

    def _new_gen(self) -> int:
        gen = self._next_gen
        self._next_gen = gen % self.GEN_MASK + 1
        return gen

    def _aborted(self) -> list:
        """Capturing slots whose done word reports the abort of their current generation."""
        d = self._edone_np
        return [s for s, (g, _) in self._capturing.items() if int(d[s]) & 0xffffffff == g | self.ENROLL_FAULT]

    def faults(self) -> list:
        """Slots the device closed (non-finite input, or an fp32 overflow inside the separator) since their last `open`, and
        idle slots whose enrollment capture it aborted (a non-finite recorded sample) since their last `enroll`."""
        f = self._fault_np
        out = [s for s, g in enumerate(self._gen) if g and int(f[s]) == g]
        if self._capturing or self._enroll_faults:
            out = sorted(set(out) | self._enroll_faults | set(self._aborted()))
        return out

    @property
    def active(self) -> list:
        """The host's view of the open slots: opened, not closed, no fault reported so far."""
        f = self._fault_np
        return [s for s, g in enumerate(self._gen) if g and int(f[s]) != g]

    @property
    def enrolling(self) -> list:
        """The slots whose clip is being recorded or embedded."""
        bad = set(self._aborted()) if self._capturing else ()
        return sorted(s for s in list(self._capturing) + list(self._embedding) if s not in bad)

    def embedding_of(self, slot: int) -> torch.Tensor:
        """The [256] device tensor `slot` was opened with by enrollment."""
        self._slot(slot)
        if slot not in self._enrolled:
            raise ValueError(f"slot {slot} was not opened by enrollment")
        return self._enrolled[slot]

    @property
    def rows_in_use(self) -> int:
        """Rows that held a listener in the last `step` (a lock-step streamer: every slot is a row)."""
        return self._n_rows if self.compact else self.S

    @property
    def last_rows(self) -> int:
        """The batch the last `step` launched its kernels for: the bucket of `rows_in_use`."""
        return self._last_rows if self.compact else self.S

    def _row(self, slot: int) -> int:
        """The row of the state buffers that holds `slot`'s listener; a compacting streamer's slot without a row: -1."""
        return self._row_of[slot] if self.compact else slot

    def _pos(self, row=None) -> tuple:
        """(pos_rows, pos_shared) as the snapshot entry points take them: the ring positions of a paced streamer's rows — all
        of them, or `row`'s own word — or the counter a lock-step streamer's rows share."""
        if not self.pace:
            return None, self._st.pos.data_ptr()
        return (self._ring[0] if row is None else self._ring[0, row:row + 1]).data_ptr(), None

    def _fresh(self, n: int) -> tuple:
        """Words on their way to the device: (src, words) — `n` zeroed int32 words in pinned host memory and the numpy view
        the caller fills before its ONE `dst.copy_(src, non_blocking=True)`.  A FRESH array per posting: the host allocator
        hands its memory out again only after the copy has run, so a host that runs ahead of the device cannot overwrite
        words in flight."""
        src = self.net._host_words(n, self.device)
        return src, src.numpy()

    def _post_words(self, dst: torch.Tensor, pending: dict):
        """{slot: word} into the [S] words `dst`, the other slots' words zero; `pending` is empty afterwards."""
        src, words = self._fresh(self.S)
        for slot, w in pending.items():
            words[slot] = w
        pending.clear()
        dst.copy_(src, non_blocking=True)

    def _set_gain(self, slot: int, embed: torch.Tensor):
        st = self._st
        st.embed[slot].copy_(embed.reshape(-1), non_blocking=True)
        row = self._row(slot)
        if row >= 0:                                        # else: `_plan` does it once the slot has a row
            self._row_gain(slot, row)

    def _row_gain(self, slot: int, row: int):
        st = self._st
        with torch.no_grad():                               # this row only, eager, stream-ordered before the next replay
            self.net._speaker_gain(st.embed[slot:slot + 1], st.gain_raw[row:row + 1], st.gain[row:row + 1])

    def _plan(self):
        """The rows of the next chunk, from the rows of the last one: listeners that left give their rows up, survivors above
        the new row count move into the holes below it, openings take the holes that are left — and the tables that tell the
        device, in one asynchronous copy."""
        f, gen, pend = self._fault_np, self._gen, self._pending
        row_of, slot_of, n_old = self._row_of, self._slot_of, self._n_rows
        for r in range(n_old):                              # closed by the host, or by the device and seen now
            s = slot_of[r]
            # ... or closed / suspended and resumed since the last step: the row is the PREVIOUS listener's.  It is given up
            # like theirs, so that the resume is an opening and takes a hole — a row kept here could be a mover of this step,
            # and the move would copy the previous listener over what `_restore` has written
            if not gen[s] or int(f[s]) == gen[s] or s in self._resumes:
                slot_of[r], row_of[s] = -1, -1
        opens = [s for s, w in pend.items() if w & self.OPEN and row_of[s] < 0]
        keep = [r for r in range(n_old) if slot_of[r] >= 0]
        n = len(keep) + len(opens)
        holes = [r for r in range(n) if r >= n_old or slot_of[r] < 0]
        movers = [r for r in reversed(keep) if r >= n]     # src >= n > dst: disjoint, one launch
        src, words = self._fresh(4 * self.S)
        words = words.reshape(4, self.S)                    # move table | row -> slot | slot -> row | cmd from the host
        for dst, r in zip(holes, movers):
            s = slot_of[r]
            slot_of[dst], row_of[s], slot_of[r] = s, dst, -1
            words[0, dst] = r + 1
        for s, dst in zip(opens, holes[len(movers):]):
            slot_of[dst], row_of[s] = s, dst
            if s not in self._resumes:                      # a resumed listener's gain follows their embedding: `_restore`
                self._row_gain(s, dst)                      # a hole or a new row: never the source of a move
        words[1], words[2] = slot_of, row_of
        for s, w in pend.items():
            if w & self.OPEN:                               # a row whose listener left needs no word: it has no slot
                words[3, row_of[s]] = w
        pend.clear()
        self._tables[:4].copy_(src.view(4, self.S), non_blocking=True)
        self._n_rows = n
        self._slot_np[:n] = slot_of[:n]
        self._rgen_np[:n] = [gen[s] for s in slot_of[:n]]
        self._rgen_np[n:] = -1

    def _check_idle(self, slot: int):
        """ValueError unless a listener can come into `slot`; an aborted capture has left the slot idle: `poll` sees that."""
        self._slot(slot)
        if slot in self.active:
            raise ValueError(f"slot {slot} is open: close() it first")
        if slot in self._capturing or slot in self._embedding:
            self.poll()
            if slot in self._capturing or slot in self._embedding:
                raise ValueError(f"slot {slot} is enrolling: close() it first")

    def _opening(self, slot: int, word: int):
        """`slot` gets a new generation, and its OPEN with that generation and `word` goes out with the next step."""
        self._enroll_faults.discard(slot)
        self._enrolled.pop(slot, None)
        gen = self._new_gen()
        # the fault word of the previous listener holds an older generation: cleared for the host as of now, and on the
        # device by the chunk that opens the slot
        self._gen[slot] = gen
        self._pending[slot] = word | self.OPEN | (gen << self.GEN_SHIFT)

    def _leave(self, slot: int):
        """The listener of `slot` leaves: idle for the host as of now, reset and closed on the device by the next step."""
        self._gen[slot] = 0
        self._enrolled.pop(slot, None)
        self._pending[slot] = self.RESET | self.CLOSE

    def _arm(self, slot: int, embedder):
        """A capture of `slot`'s next `enroll_chunks` chunks, under a generation of its own, starts with the next step."""
        gen = self._new_gen()
        self._capturing[slot] = (gen, embedder)
        self._epending[slot] = self.ARM | (gen << self.GEN_SHIFT)

    def _open(self, slot: int, embed: torch.Tensor):
        self._opening(slot, self.RESET)
        self._set_gain(slot, embed)

    def open(self, slot: int, embed: torch.Tensor):
        """From the next `step` on `slot` is a fresh stream that listens for `embed` [256]."""
        self._check_idle(slot)
        self._open(slot, embed)

    def enroll(self, slot: int, embedder, passthrough: bool = False):
        """From the next `step` on the rows of idle `slot` are recorded, `enroll_chunks` of them; then
        `embedder(clips [k, 2, 128 enroll_chunks]) -> [k, 256]` (an `EmbedTFGridNet` on this device) runs beside the chunk
        loop and the slot opens on its row.  Until then the slot's output rows are zeros — or, with `passthrough` (a monitor
        streamer), the listener's own input: the slot's mix goes to (0, 1) with the arming and back to (1, 0) in the step
        that opens the slot, so the room cross-fades into the target on the slot's first live chunk.  A capture that is
        aborted or cancelled leaves the mix where it is: the listener keeps the room until `set_mix` says otherwise."""
        self._slot(slot)
        if not self.enroll_chunks:
            raise ValueError("this SessionStreamer was built without enrollment: make_session_streamer(..., enroll_chunks=n)")
        if passthrough and not self.monitor:
            raise ValueError("passthrough is the dry path of a monitor streamer: make_session_streamer(..., monitor=True)")
        self.poll()
        if slot in self.active:
            raise ValueError(f"slot {slot} is open: close() it first")
        if slot in self._capturing or slot in self._embedding:
            raise ValueError(f"slot {slot} is enrolling already")
        self._gen[slot] = 0                                 # a slot the device closed for a fault is idle there already
        self._enroll_faults.discard(slot)
        self._enrolled.pop(slot, None)
        self._arm(slot, embedder)
        self._passthrough.discard(slot)
        if passthrough:
            self.set_mix(slot, 0.0, 1.0)
            self._passthrough.add(slot)

    def relook(self, slot: int, embedder):
        """"Look once" at another speaker without leaving the session: from the next `step` on the rows of OPEN `slot` are
        recorded as `enroll` records an idle slot's, while the separator goes on with the current embedding — the slot stays
        in `active` (and is listed by `enrolling` too), keeps its row in a compacting streamer, and its output is bit for bit
        what it would be without the capture.  The finished embedding takes the `set_embedding` path: the carried state is
        kept, `embedding_of(slot)` is the new one.  `close` cancels the look and closes the session; an aborted capture leaves
        the old target in place (the non-finite input faults the session anyway); `suspend` is refused meanwhile."""
        self._slot(slot)
        if not self.enroll_chunks:
            raise ValueError("this SessionStreamer was built without enrollment: make_session_streamer(..., enroll_chunks=n)")
        self.poll()
        if slot in self._capturing or slot in self._embedding:
            raise ValueError(f"slot {slot} is enrolling already")
        if slot not in self.active:
            raise ValueError(f"slot {slot} is not open: enroll() it")
        self._arm(slot, embedder)
        self._relook.add(slot)

    def close(self, slot: int):
        """From the next `step` on `slot` is idle: its output rows are exact zeros.  Also acknowledges a fault, and cancels an
        enrollment in progress: nothing opens later.  A `relook` is cancelled and its session closed."""
        self._slot(slot)
        if slot in self._capturing or slot in self._embedding:
            if self._capturing.pop(slot, None) is not None:
                self._epending[slot] = self.CANCEL
            self._embedding.pop(slot, None)                 # the call goes on; its row is dropped by generation
            self._passthrough.discard(slot)
            if slot not in self._relook:
                return
            self._relook.discard(slot)                      # ... and the session it ran beside is closed below
        if slot in self._enroll_faults:
            self._enroll_faults.discard(slot)
            return
        if not self._gen[slot]:
            raise ValueError(f"slot {slot} is not open")
        self._resumes.pop(slot, None)                       # resumed and closed before a `step`: nothing is restored
        self._leave(slot)

    def _snap_args(self, k: int, slot=None):
        """The leading arguments of lh_session_save / lh_session_restore up to the embedding: ping-pong set k, `slot`; of the
        *_rows forms without a slot: the embeddings of all slots."""
        live, rings, emb = self._spans_live[k], self._spans_rings, self._st.embed
        return (ctypes.addressof(live), len(live), ctypes.addressof(rings), len(rings), *self._ring_geom,
                (emb if slot is None else emb[slot]).data_ptr(), emb.shape[1] * emb.element_size())

    def _suspendable(self, slot: int):
        self._slot(slot)
        if slot in self._capturing or slot in self._embedding:
            raise ValueError(f"slot {slot} is enrolling: it has no session yet")
        if slot not in self.active:
            raise ValueError(f"slot {slot} is not open")
        if slot in self._pending:
            raise ValueError(f"slot {slot} was opened or resumed and no step has served it yet: it has no state on the device")

    def suspend(self, slot: int) -> SessionSnapshot:
        """The listener of open `slot` as a `SessionSnapshot`: their state as of the last `step`.  From the next `step` on the
        slot is idle exactly as after `close(slot)`.  Enqueues one launch and returns; never waits for the device."""
        self._suspendable(slot)
        st, net, row, words = self._st, self.net, self._row(slot), self._words
        pos_row, pos_shared = self._pos(row)                # the word that holds this row's ring position: either one
        data = torch.empty(self._snap_bytes, dtype=torch.uint8, device=self.device)
        with torch.no_grad(), net._device_ctx(st.chunk):
            # the set the next chunk reads is the one the last chunk wrote: sets[parity]
            net._lib(st.chunk).call("lh_session_save", *self._snap_args(st.parity, slot), data.data_ptr(), self._snap_bytes,
                                    words.data_ptr(), words[2].data_ptr(), pos_shared if pos_row is None else pos_row, row, self.S,
                                    net._stream(self.device))
            event = net._record_event(self.device)
        self._leave(slot)
        return SessionSnapshot(data, self._snap_layout, event)

    def _items(self, items: list) -> torch.Tensor:
        """A table of lh_snap_item_t (row, slot, generation, index) on the device, posted as the command words are."""
        src, words = self._fresh(4 * len(items))
        words.reshape(-1, 4)[:] = items
        table = torch.empty(len(items), 4, dtype=torch.int32, device=self.device)
        table.copy_(src.view(-1, 4), non_blocking=True)
        return table

    def suspend_many(self, slots) -> "SessionSnapshotBatch":
        """`suspend(s)` for every s of `slots`, in order, between the same two steps — the same snapshot bytes, the same slots idle
        afterwards — as ONE launch (`lh_session_save_rows`) into one fresh [k, snapshot bytes] tensor, behind one asynchronous
        copy of the item table.  Every ValueError of `suspend` applies, a slot named twice is one more; everything is checked
        before anything is enqueued or changed.  Never waits for the device."""
        slots = [int(s) for s in slots]
        for slot in slots:
            self._suspendable(slot)
        if len(set(slots)) != len(slots):
            raise ValueError(f"a slot is named twice: {slots}")
        st, net, k, words = self._st, self.net, len(slots), self._words
        data = torch.empty(k, self._snap_bytes, dtype=torch.uint8, device=self.device)
        event = None
        if k:
            items = self._items([(self._row(s), s, 0, i) for i, s in enumerate(slots)])
            with torch.no_grad(), net._device_ctx(st.chunk):
                net._lib(st.chunk).call("lh_session_save_rows", *self._snap_args(st.parity), data.data_ptr(), data.stride(0),
                                        words.data_ptr(), words[2].data_ptr(), *self._pos(), items.data_ptr(), k, self.S,
                                        net._stream(self.device))
                event = net._record_event(self.device)
        for slot in slots:
            self._leave(slot)
        return SessionSnapshotBatch(data, self._snap_layout, event)

    def drain(self):
        """Everyone leaves: (the active slots in ascending order, `suspend_many` of them)."""
        slots = self.active
        return slots, self.suspend_many(slots)

    def _resumable(self, slot: int, layout: tuple, nbytes: int):
        self._check_idle(slot)
        if layout != self._snap_layout or nbytes != self._snap_bytes:
            raise ValueError(f"the snapshot's layout {layout} ({nbytes} bytes) is not this Net's "
                             f"{self._snap_layout} ({self._snap_bytes} bytes)")

    def _resumed(self, slot: int, snapshot: SessionSnapshot) -> list:
        # no RESET: lh_session_restore writes every byte a RESET would zero, apart from what the chunk rewrites itself
        self._opening(slot, 0)
        self._resumes[slot] = entry = [snapshot, None]
        return entry

    def resume(self, slot: int, snapshot: SessionSnapshot):
        """From the next `step` on idle `slot` is the listener of `snapshot`: carried state, ring history, ring position and
        speaker embedding are theirs (there is no embedding argument).  ValueError for a snapshot of another model layout.
        Never waits for the device: a snapshot in another GPU's memory is copied over behind its event."""
        self._resumable(slot, snapshot.layout, snapshot.data.numel())
        self._resumed(slot, snapshot.to(self.device))

    def resume_many(self, slots, snapshots):
        """`resume(slots[i], snapshots[i])` for every i, in order — the generations handed out, `set_embedding` and `close`
        afterwards, dead snapshots, a compacting streamer's holes: all as there — but `step` restores them in ONE launch
        (`lh_session_restore_rows`) and computes their gains in one call.  `snapshots`: a `SessionSnapshotBatch`, or a sequence
        of `SessionSnapshot`; views of one batch use that batch in place (any subset, any order), anything else is stacked
        first.  A batch in another GPU's memory comes over in one copy behind its event.  Everything is checked before anything
        changes: a slot named twice, an open or enrolling slot and another model's layout are ValueErrors.  Never waits."""
        slots = [int(s) for s in slots]
        if isinstance(snapshots, SessionSnapshotBatch):
            batch, index = snapshots, list(range(len(snapshots)))
            layouts = [(batch.layout, batch.nbytes)] * len(index)
        else:
            snaps = list(snapshots)
            batch = snaps[0].batch if snaps and all(sn.batch is snaps[0].batch for sn in snaps) else None
            index = [sn.index for sn in snaps] if batch is not None else list(range(len(snaps)))
            layouts = [(sn.layout, sn.data.numel()) for sn in snaps]
        if len(slots) != len(index):
            raise ValueError(f"{len(slots)} slots for {len(index)} snapshots")
        if len(set(slots)) != len(slots):
            raise ValueError(f"a slot is named twice: {slots}")
        for slot, (layout, nbytes) in zip(slots, layouts):
            self._resumable(slot, layout, nbytes)
        if not slots:
            return
        batch = SessionSnapshotBatch.stack(snaps, self.device) if batch is None else batch.to(self.device)
        self._resume_batches.append((batch, {slot: (i, self._resumed(slot, batch[i])) for slot, i in zip(slots, index)}))

    def _restore(self):
        """The resumes of this step, behind the copy of the command words (a dead snapshot takes its OPEN back) and ahead of
        the chunk.  The rows are idle, and in a compacting streamer holes: no move of the step reads or writes them."""
        st, net, S, words = self._st, self.net, self.S, self._words
        with torch.no_grad(), net._device_ctx(st.chunk):
            lib, stream = net._lib(st.chunk), net._stream(self.device)
            # `resume_many`: the slots of a batch that still hold that resume (not closed, or closed and resumed again, since)
            groups = [(batch, [(slot, i) for slot, (i, entry) in group.items() if self._resumes.get(slot) is entry])
                      for batch, group in self._resume_batches]
            batched = {slot for _, live in groups for slot, _ in live}
            for slot, (snap, embed) in self._resumes.items():
                if slot in batched:
                    continue
                row = self._row(slot)
                net._wait_event(self.device, snap.event, snap.data)
                lib.call("lh_session_restore", *self._snap_args(st.parity, slot), snap.data.data_ptr(), snap.data.numel(),
                         words.data_ptr(), *self._pos(row), self._fault[slot:slot + 1].data_ptr(), self._gen[slot], row, S,
                         stream)
                if embed is not None:                       # `set_embedding` after `resume`
                    st.embed[slot].copy_(embed.reshape(-1), non_blocking=True)
                self._row_gain(slot, row)
            for batch, live in groups:                      # one table, one restore launch, one gain call per batch
                if not live:
                    continue
                net._wait_event(self.device, batch.event, batch.data)
                items = self._items([(self._row(slot), slot, self._gen[slot], i) for slot, i in live])
                lib.call("lh_session_restore_rows", *self._snap_args(st.parity), batch.data.data_ptr(), batch.data.stride(0),
                         words.data_ptr(), *self._pos(), self._fault.data_ptr(), items.data_ptr(), len(live), S, stream)
                for slot, _ in live:
                    embed = self._resumes[slot][1]
                    if embed is not None:                   # `set_embedding` after `resume_many`
                        st.embed[slot].copy_(embed.reshape(-1), non_blocking=True)
                net._speaker_gain_rows(st.embed, st.gain_raw, st.gain, items)
        self._resumes.clear()
        self._resume_batches.clear()

    def _packet_streamer(self):
        if not self.packets:
            raise ValueError("this SessionStreamer takes windows: make_session_streamer(..., pace=True, packets=True)")

    def buffered(self, slot: int) -> int:
        """Samples pushed for `slot` and not yet consumed by a `step` (host arithmetic; a pending `flush` counts as done)."""
        self._packet_streamer()
        slot = self._slot(slot)
        return 0 if slot in self._flush else (self._wr[slot] - self._rd[slot]) & self.COUNTER_MASK

    def ready(self) -> list:
        """The slots that hold a whole window, 192 samples: the next `step` consumes a chunk of each (host arithmetic)."""
        self._packet_streamer()
        return [s for s in range(self.S) if self.buffered(s) >= self.WINDOW]

    def flush(self, slot: int):
        """Drops what `slot` has buffered: a host that gives the slot to another client does this.  Travels with the slot's
        item of the next `push`, or in a push of its own that the next `step` issues."""
        self._packet_streamer()
        self._flush.add(self._slot(slot))

    # The FIFO's counters on the host, in the integers of lh_stream.hip: `_admit` is what lh_session_feed and
    # lh_session_resample_in will find, `_framed` what lh_session_frame will find and do.  Nothing is read back.
    def _admit(self, packets: dict) -> list:
        """`push`, before anything changes: [(slot, samples, n, 16 kHz blocks the resampler will make of them)] for the slots
        that get a feed item, or the error.  A 16 kHz streamer's FIFO gets the n samples themselves and makes no blocks; a
        `client_rate` streamer's gets the blocks whose K taps are complete in the raw ring once the n samples are there."""
        M, R, flushed, resamp = self.COUNTER_MASK, self.fifo_samples, self._flush, self._resampling
        dtype, nch, wr, rd = torch.int16 if self.pcm16 else torch.float32, self.chunk_in.shape[1], self._wr, self._rd
        if resamp:
            raw_wr, tap, tap0, o, nn, K = self._raw_wr, self._tap, self._tap0, self._o_in, self._n_in, self._k_in
        todo = []
        for slot, x in packets.items():
            slot = self._slot(int(slot))
            if not isinstance(x, torch.Tensor) or x.is_cuda or x.dtype != dtype or x.dim() != 2 or x.shape[0] != nch:
                raise ValueError(f"slot {slot}: a packet is a CPU {dtype} tensor [{nch}, n]")
            n, fl, blocks = x.shape[1], slot in flushed, 0
            have = 0 if fl else (wr[slot] - rd[slot]) & M
            made = n
            if resamp:
                fill = ((0 if fl else raw_wr[slot]) + n - (tap0 if fl else tap[slot])) & M
                blocks = 0 if fill < K else (fill - K) // o + 1
                made = blocks * nn
            if have + made > R:
                what, rate = (f"{made} made of the {n} pushed", " (at 16 kHz)") if resamp else (f"{n} pushed", "")
                raise BufferError(f"slot {slot}: {have} samples buffered + {what} > fifo_samples = {R}{rate}: "
                                  "step() first (while ss.ready(): ss.step()), or flush(slot)")
            if n or fl:
                todo.append((slot, x, n, blocks))
        if flushed:                                         # a flush without a packet travels in an item of its own
            todo += [(slot, None, 0, 0) for slot in sorted(flushed - {t[0] for t in todo})]
        return todo

    def _framed(self) -> tuple:
        """One chunk of every slot that holds a window: who that is, with their read counters a hop further."""
        wr, rd, M = self._wr, self._rd, self.COUNTER_MASK
        took = tuple((w - r) & M >= self.WINDOW for w, r in zip(wr, rd))
        for s, t in enumerate(took):
            if t:
                rd[s] = (rd[s] + self.HOP) & M
        return took

    def _counted(self, took: tuple) -> tuple:
        """What lh_session_resample_out_any will count for the slots that took a chunk, c(r + 1) - c(r) client samples at phase
        r, with their phases a step further."""
        ph, o, n, P, H = self._phase_of, self._o_out, self._n_out, self._period, self.HOP
        counts = [0] * self.S
        for s, t in enumerate(took):
            if t:
                r = ph[s]
                counts[s] = H * (r + 1) * n // o - H * r * n // o
                ph[s] = (r + 1) % P
        return tuple(counts)

    @property
    def last_counts(self) -> tuple:
        """The valid samples of each slot's row of the last `step` (host arithmetic): 0 for a slot that was held, else 128, the
        `hop_client` of a fixed-hop client rate, or with `any_rate` the floor or ceil of 128 rate / 16000 that the slot's phase
        makes it — the columns behind it are zeros."""
        self._packet_streamer()
        if self._fractional:
            return self._last_counts
        return tuple(self.hop_client if t else 0 for t in self.last_present)

    def push(self, packets: dict):
        """packets {slot: CPU tensor [2, n]}, float32 (int16 in a `pcm16` streamer), any n >= 0: the clients' contiguous PCM
        as it arrived since the last call.  One fresh pinned buffer (item table, then the samples), one asynchronous copy
        and one `lh_session_feed` launch, whatever the number of packets; never waits for the device.  BufferError, before
        anything is enqueued or changed for any slot, when a slot would hold more than `fifo_samples`.
        A `client_rate` streamer takes the samples at the client's rate: they go to the slot's raw ring, and a second launch
        (`lh_session_resample_in`) makes the 16 kHz blocks whose taps are now complete — `fifo_samples` bounds those."""
        self._packet_streamer()
        todo = self._admit(packets)
        if todo:
            self._feed(*self._staged(todo))

    def _staged(self, todo: list) -> tuple:
        """`push`, once everything is admitted: the feed items, the resample items and the samples in one posting to `_stage`,
        the host's counters moved as the device will move its own.  -> (samples, feed items, resample items)."""
        M, nch, flushed, resamp = self.COUNTER_MASK, self.chunk_in.shape[1], self._flush, self._resampling
        wr16, rd = self._wr, self._rd
        wr = self._raw_wr if resamp else wr16               # the ring the feed serves; wr16 / rd stay the FIFO's
        per = 2 if self.pcm16 else 1                        # samples per 32-bit word
        total = sum(nch * n for _, _, n, _ in todo)
        i32 = lambda v: v - (1 << 32) if v >> 31 else v       # a 32-bit pattern as an int32 table holds it
        off, ritems = 0, []
        used = self._item_words + (total + per - 1) // per
        src, buf = self._fresh(used)
        table = buf[:self.FEED_ITEM_WORDS * len(todo)].reshape(-1, self.FEED_ITEM_WORDS)
        samples = buf[self._item_words:].view(np.int16 if self.pcm16 else np.float32)
        for i, (slot, x, n, blocks) in enumerate(todo):
            flush = slot in flushed
            if flush:
                wr[slot] = rd[slot] = 0
                if resamp:                                  # the stream restarts from silence: zero history, phase 0
                    wr16[slot], self._tap[slot] = 0, self._tap0
                    for t in (self._raw[slot], self._tail[slot], self._fifo_words[:, slot]):
                        t.zero_()
                    if self._fractional:
                        self._phase_of[slot] = 0
                        self._phase[slot].zero_()
            at = wr[slot]
            table[i] = (slot, off, n, i32(at), self.FEED_FLUSH if flush else 0)
            if n:
                samples[off:off + nch * n].reshape(nch, n)[...] = x.numpy()
            wr[slot] = (at + n) & M
            off += nch * n
            if blocks:
                tap = self._tap[slot]
                ritems.append((slot, blocks, i32(wr16[slot]), i32(tap)))
                wr16[slot], self._tap[slot] = (wr16[slot] + blocks * self._n_in) & M, (tap + blocks * self._o_in) & M
        flushed.clear()
        if ritems:
            buf[self._ritem_off:self._ritem_off + self.RESAMPLE_ITEM_WORDS * len(ritems)].reshape(
                -1, self.RESAMPLE_ITEM_WORDS)[...] = ritems
        self._stage[:used].copy_(src, non_blocking=True)
        return total, len(todo), len(ritems)

    def _feed(self, total: int, n_items: int, n_ritems: int):
        """The launches of a `push` behind its posting: the feed into the ring the clients write to, then the resampler's."""
        net, st, S, R = self.net, self._st, self.S, self.fifo_samples
        ring, words, Rr = (self._raw, self._raw_words, self.raw_samples) if self._resampling else (self._fifo, self._fifo_words, R)
        with torch.no_grad(), net._device_ctx(st.chunk):
            lib, stream = net._lib(st.chunk), net._stream(self.device)
            lib.call("lh_session_feed", self._stage[self._item_words:].data_ptr(), total * (2 if self.pcm16 else 4),
                     self.FEED_S16 if self.pcm16 else self.FEED_F32, self._stage.data_ptr(), n_items, ring.data_ptr(),
                     words[0].data_ptr(), words[1].data_ptr(), Rr, S, stream)
            if n_ritems:
                lib.call("lh_session_resample_in", ring.data_ptr(), Rr, self._stage[self._ritem_off:].data_ptr(), n_ritems,
                         self._fifo.data_ptr(), self._fifo_words[0].data_ptr(), R, S, self._bank_in.data_ptr(), self._o_in,
                         self._n_in, self._w_in, stream)

    def set_embedding(self, slot: int, embed: torch.Tensor):
        """Re-target an open slot ("look once" at another speaker): the carried state is kept."""
        self._slot(slot)
        if not self._gen[slot]:
            raise ValueError(f"slot {slot} is not open")
        if slot in self._resumes:                           # the snapshot's embedding is not there yet: after the restore
            self._resumes[slot][1] = embed
            return
        self._set_gain(slot, embed)

    def poll(self):
        """Moves enrollments on, without waiting for the device: clips the device has completed go to the embedder on the side
        stream, finished embeddings open their slots.  `step` calls it first; call it more often if you like."""
        if not self._capturing and not self._jobs:
            return
        d, ready = self._edone_np, {}
        for s in sorted(self._capturing):
            g, embedder = self._capturing[s]
            w = int(d[s]) & 0xffffffff
            if w == g:
                ready.setdefault(embedder, []).append(s)
            elif w == g | self.ENROLL_FAULT:
                del self._capturing[s]
                self._passthrough.discard(s)                # the mix stays: the listener keeps the room
                if s in self._relook:                       # the session has its own fault word; the old target stays
                    self._relook.discard(s)
                else:
                    self._enroll_faults.add(s)
        for embedder, slots in ready.items():               # one call per embedder: a batch in ascending slot order
            gens = [self._capturing.pop(s)[0] for s in slots]
            # views and a copy on the side stream: nothing here moves host memory, so nothing waits
            clips = lambda: self._clips[slots[0]:slots[0] + 1] if len(slots) == 1 else torch.stack([self._clips[s] for s in slots])
            with torch.no_grad():
                out, done = self._side.run(lambda: embedder(clips()))
            self._embedding.update(zip(slots, gens))
            self._jobs.append((done, slots, gens, out))
        while self._jobs and self._side.finished(self._jobs[0][0]):      # one stream: the calls finish in order
            done, slots, gens, out = self._jobs.pop(0)
            self._side.hand_over(done, out)
            for i, s in enumerate(slots):
                if self._embedding.get(s) == gens[i]:       # else: cancelled (and perhaps enrolling again) meanwhile
                    del self._embedding[s]
                    if s in self._relook:                   # the session goes on: `set_embedding`, state kept
                        self._relook.discard(s)
                        if s in self.active:                # else the device closed it meanwhile: nothing to re-target
                            self._enrolled[s] = out[i]
                            self.set_embedding(s, out[i])
                        continue
                    self._open(s, out[i])
                    self._enrolled[s] = out[i]              # behind the opening, which forgets the slot's previous one
                    if s in self._passthrough:              # with the OPEN: the cross-fade starts on the first live chunk
                        self._passthrough.discard(s)
                        self.set_mix(s, 1.0, 0.0)

    def step(self, chunks: Optional[torch.Tensor] = None, present=None) -> torch.Tensor:
        """chunks [S, 2, 192] (rows of idle slots are ignored) -> [S, 2, 128] (rows of idle slots are zeros); a view the next
        `step` overwrites.  Never raises for a slot's fault: see `faults()`.
        `present` (a paced streamer only): a length-S sequence or CPU bool tensor, false = the slot is held for this step —
        its row of `chunks` is ignored, its output row is zeros, its state stays.  None: everyone is present.
        A packet streamer takes neither: `step()` consumes one window of every slot that has 192 samples buffered, holds the
        others, and says which in `last_present`; the output is int16 when the streamer was built with `pcm16`."""
        st = self._st
        if self.packets:
            if chunks is not None or present is not None:
                raise ValueError("a packet streamer gets its samples through push(): step() takes no chunks and no `present`")
        elif chunks is None:
            raise ValueError("step() without chunks needs a packet streamer: make_session_streamer(..., pace=True, packets=True)")
        if present is not None and not self.pace:
            raise ValueError("`present` needs a paced streamer: make_session_streamer(..., pace=True)")
        st._check_repacked()
        st._check_versions()
        self.poll()
        if self.packets:
            if self._flush:                                 # a flush nobody pushed behind travels on its own
                self.push({})
            self.last_present = self._framed()              # the device frames and holds by itself: no hold word travels
            if self._fractional:
                self._last_counts = self._counted(self.last_present)
        elif self.pace:
            held = self._none_held
            if present is not None:
                held = tuple(not p for p in (present.tolist() if isinstance(present, torch.Tensor) else present))
                if len(held) != self.S:
                    raise ValueError(f"`present` has {len(held)} entries for {self.S} slots")
            if held != self._held:                          # a steady loop copies nothing
                src, words = self._fresh(self.S)
                words[:] = held
                self._hold.copy_(src, non_blocking=True)
                self._held = held
        if self.compact:
            n = self._n_rows
            if self._pending or (n and (self._fault_np[self._slot_np[:n]] == self._rgen_np[:n]).any()):
                self._plan()
            self._last_rows = next(b for b in self.row_buckets if b >= self._n_rows)
        elif self._pending:
            self._post_words(self._words[0], self._pending)
        if self._epending:                                  # the LH_ENROLL_* words travel the same way
            self._post_words(self._ewords[0], self._epending)
        if self.monitor and not self._mix_posted:           # the mix targets too: bit patterns of fp32, [2][S]
            src, words = self._fresh(2 * self.S)
            words.view(np.float32).reshape(2, self.S)[:] = np.asarray(self._targets, dtype=np.float32).T
            self._mix[0].view(torch.int32).copy_(src.view(2, self.S), non_blocking=True)
            self._mix_posted = True
        if self._resumes:
            self._restore()
        if not self.packets:
            self.chunk_in.copy_(chunks)
        with torch.no_grad():
            if self.graphs is None:
                self._body(st.parity, self.last_rows)
            elif self.compact:
                self.graphs[self._last_rows][st.parity].replay()
            else:
                self.graphs[st.parity].replay()
        st.parity ^= 1
        if self._resampling:
            return self.out_client
        return self.out16 if self.pcm16 else self.out
