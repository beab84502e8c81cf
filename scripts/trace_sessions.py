"""Launch-for-launch trace of `SessionStreamer`'s host code, to compare two trees of this repository on the CPU.

    python scripts/trace_sessions.py --out FILE

drives a `SessionStreamer` of 3 slots on "cpu", eager, in every flavour, through a fixed script of public calls over a
RECORDING stand-in for the library: `call` and `raw` write down what they are given and return 0, nothing executes.  The
words the device would write (`_fault`, `_edone`) are poked by hand where the script says so, so the host branches that
react to them run.  Run it in two worktrees and `cmp` the files: a host-side refactor leaves them identical.

One JSON line per public call:
  * `lib`: every library call in order — name, integers and floats exact, None as such, every pointer as
    [buffer, byte offset], every `lh_span_t` array expanded to its [buffer, offset, bytes] entries;
  * `ops`: every in-place torch op (the copies, the zeroing) with its tensors as [buffer, offset, shape, strides, dtype];
  * `words`: every `_host_words` allocation — its length and what it holds when the public call returns;
  * `ret` or `exc` (type and message), and after a `step` the streamer's public view of itself.
A buffer is named by the rank of first appearance of its storage among everything recorded in its flavour, never by an
attribute name: `buf` was allocated by the constructor, `in` by this script between two calls, `new` inside a public
call (snapshot data, item tables, host words)."""
import argparse
import bisect
import contextlib
import ctypes
import json
import os
import sys

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lookoncetohear_amd import _cabi, config                                    # noqa: E402
from lookoncetohear_amd.net import Net, SessionSnapshot, SessionSnapshotBatch    # noqa: E402

S = 3
FAULT = 0x80000000                                          # LH_ENROLL_FAULT


class Tracer(TorchDispatchMode):
    """The registry of every storage seen (kept alive, so that no address is handed out twice) and the record of the
    public call in progress."""

    def __init__(self):
        super().__init__()
        self.storages, self.bases = {}, None                # base -> (bytes, phase, a tensor that keeps it alive)
        self.phase, self.rank, self.spans = "buf", {}, {}
        self.event = None

    # ---- storages ----------------------------------------------------------------------------------------------------
    def see(self, t):
        st = t.untyped_storage()
        base, n = st.data_ptr(), st.nbytes()
        if n and base not in self.storages:
            self.storages[base] = (n, self.phase, t)
            self.bases = None

    def where(self, ptr):
        """[buffer, byte offset] of an address."""
        if self.bases is None:
            self.bases = sorted(self.storages)
        i = bisect.bisect_right(self.bases, ptr) - 1
        if i >= 0 and ptr < self.bases[i] + self.storages[self.bases[i]][0]:
            base = self.bases[i]
            rank = self.rank.setdefault(base, len(self.rank))
            return [f"{self.storages[base][1]}{rank}", ptr - base]
        return ["unknown", 0]

    def tensor(self, t):
        self.see(t)
        return self.where(t.data_ptr()) + [list(t.shape), list(t.stride()), str(t.dtype)] if t.numel() else ["empty", list(t.shape)]

    def find_spans(self, obj, seen=None):
        """Every ctypes array of (base, bytes) structures reachable from `obj`, by address."""
        seen = set() if seen is None else seen
        if id(obj) in seen:
            return
        seen.add(id(obj))
        if isinstance(obj, ctypes.Array):
            if hasattr(obj._type_, "_fields_"):
                self.spans[ctypes.addressof(obj)] = obj
        elif isinstance(obj, (list, tuple, set)):
            for x in obj:
                self.find_spans(x, seen)
        elif isinstance(obj, dict):
            for x in obj.values():
                self.find_spans(x, seen)
        elif type(obj).__module__.startswith("lookoncetohear_amd") and not isinstance(obj, torch.nn.Module):
            self.find_spans(vars(obj), seen)

    # ---- what is recorded --------------------------------------------------------------------------------------------
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        flat = tree_flatten((args, kwargs, out))[0]
        for x in flat:
            if isinstance(x, torch.Tensor):
                self.see(x)
        if self.event is not None and func._schema.is_mutable:
            plain = lambda x: x if isinstance(x, (int, float, bool, str, type(None))) else str(x)
            self.event["ops"].append([str(func)] + [self.tensor(x) if isinstance(x, torch.Tensor) else plain(x)
                                                    for x in tree_flatten((args, kwargs))[0]])
        return out

    def lib_call(self, name, args):
        types, rec = _cabi.SIGNATURES[name], [name]
        assert len(types) == len(args), name
        for ty, a in zip(types, args):
            if ty is not ctypes.c_void_p or a is None or a == 0:
                rec.append(a)
            elif a in self.spans:
                rec.append([self.where(sp.base) + [sp.bytes] for sp in self.spans[a]])
            else:
                rec.append(self.where(a))
        if self.event is not None:
            self.event["lib"].append(rec)

    def value(self, v):
        if isinstance(v, torch.Tensor):
            return self.tensor(v)
        if isinstance(v, (SessionSnapshot, SessionSnapshotBatch)):
            return [type(v).__name__, self.tensor(v.data), list(v.layout), v.event is not None]
        if isinstance(v, (list, tuple)):
            return [self.value(x) for x in v]
        if isinstance(v, dict):
            return {str(k): self.value(x) for k, x in v.items()}
        return v if isinstance(v, (int, float, bool, str, type(None))) else type(v).__name__


class RecLib:
    """The library: every entry point is written down and returns 0."""

    def __init__(self, tracer):
        self.tracer = tracer

    def call(self, name, *args):
        self.tracer.lib_call(name, args)

    def raw(self, name):
        def fn(*args):
            self.tracer.lib_call(name, [getattr(a, "value", a) for a in args])
            return 0
        return fn


class SyncSide:
    """The enrollment side stream: the embedder runs inline.  `hold` keeps its call "in flight"."""
    hold = False

    def run(self, fn):
        return fn(), None

    def finished(self, done):
        return not self.hold

    def hand_over(self, done, out):
        pass


def make_net(tracer):
    class TraceNet(Net):                                    # the host of tests/hipemu/hosts.py, over the recorder
        def _lib(self, t):
            assert not t.is_cuda
            return self.emu_lib

        def _stream(self, device):
            return 0

        def _device_ctx(self, t):
            return contextlib.nullcontext()

        def _flag_words(self, device):
            return torch.zeros(2, dtype=torch.int32)

        def _host_words(self, n, device):
            t = torch.zeros(n, dtype=torch.int32)
            tracer.see(t)
            if tracer.event is not None:
                tracer.event["_words"].append(t)
            return t

        def _enroll_side(self, dev):
            return SyncSide()

        def _record_event(self, device):
            return None

        def _wait_event(self, device, ev, tensor=None):
            assert ev is None

        def _sync(self, dev):
            pass

        def _capturing(self):
            return False

    torch.manual_seed(0)
    net = TraceNet(**config.TSH_PARAMS).eval()
    net.emu_lib = RecLib(tracer)
    return net


class Flavour:
    """One streamer and the script's handle on it: every public call goes through `do`."""

    def __init__(self, tracer, net, name, out, **kw):
        self.t, self.name, self.out, self.kw, self.n_calls, self.n_lib = tracer, name, out, kw, 0, 0
        tracer.rank, tracer.spans, tracer.phase = {}, {}, "buf"
        self.record("make_session_streamer", lambda: net.make_session_streamer(S, "cpu", use_graph=False, **kw), [kw])
        self.ss = self.last
        tracer.find_spans(self.ss)
        tracer.find_spans(self.ss._st)
        self.embeds = 0

    def record(self, op, fn, args):
        t = self.t
        t.event = ev = {"flavour": self.name, "op": op, "args": t.value(args), "lib": [], "ops": [], "_words": []}
        self.last = None
        try:
            if op != "make_session_streamer":
                t.phase = "new"
            self.last = fn()
            ev["ret"] = t.value(self.last)
        except Exception as e:                              # part of the contract: type and message
            ev["exc"] = [type(e).__name__, str(e)]
        finally:
            t.event, t.phase = None, "in"
        ev["words"] = [[w.numel(), w.tolist()] for w in ev.pop("_words")]
        ss = getattr(self, "ss", None)
        if op == "step" and ss is not None:
            ev["after"] = dict(active=ss.active, faults=ss.faults(), enrolling=ss.enrolling, rows_in_use=ss.rows_in_use,
                               last_rows=ss.last_rows, last_present=t.value(getattr(ss, "last_present", None)))
        self.n_calls += 1
        self.n_lib += len(ev["lib"])
        self.out.write(json.dumps(ev) + "\n")
        return self.last

    def do(self, op, *args, **kw):
        return self.record(op, lambda: getattr(self.ss, op)(*args, **kw), [list(args), kw])

    def get(self, name):
        return self.record(name, lambda: getattr(self.ss, name), [])

    # ---- the script's inputs -------------------------------------------------------------------------------------------
    def embed(self):
        self.embeds += 1
        return torch.full((256,), float(self.embeds))

    def embedder(self, clips):
        """Stands for an `EmbedTFGridNet`: [k, 2, n] -> [k, 256]."""
        return torch.full((clips.shape[0], 256), float(clips.shape[0]))

    def step(self, present=None):
        if self.kw.get("packets"):
            return self.do("step")
        chunks = torch.zeros(S, 2, 192)
        return self.do("step", chunks) if present is None else self.do("step", chunks, present)

    def packet(self, n):
        return torch.zeros(2, n, dtype=torch.int16 if self.kw.get("pcm16") else torch.float32)

    def feed(self):
        """A packet streamer gets a window's worth for everyone, so that the steps that follow consume chunks."""
        if self.kw.get("packets"):
            n = 128 * self.ss.client_rate // 16000
            self.do("push", {s: self.packet(n) for s in range(S)})


def script(f):
    ss, kw = f.ss, f.kw
    enroll, monitor, pace, packets = kw.get("enroll_chunks", 0), kw.get("monitor", False), kw.get("pace", False), \
        kw.get("packets", False)
    # open two slots, re-target one, close the lower one (a compacting streamer moves the other), open into the hole
    f.do("open", 0, f.embed())
    f.do("open", 1, f.embed())
    f.do("open", 1, f.embed())                              # ValueError: open
    f.do("open", S, f.embed())                              # IndexError
    f.do("suspend", 1)                                      # ValueError: no step has served it
    f.feed()
    f.step()
    f.do("set_embedding", 1, f.embed())
    f.do("set_embedding", 2, f.embed())                     # ValueError: not open
    f.step()
    f.do("close", 0)
    f.do("close", 0)                                        # ValueError: not open
    f.feed()
    f.step()
    f.do("open", 0, f.embed())
    f.step()
    # the device closes slot 1: its fault word holds its generation
    ss._fault_np[1] = ss._gen[1]
    f.do("faults")
    f.get("active")
    f.feed()
    f.step()
    f.do("close", 1)
    f.step()
    # suspend, resume elsewhere, re-target before the step that restores
    f.do("open", 1, f.embed())
    f.step()
    snap = f.do("suspend", 0)
    f.do("suspend", 0)                                      # ValueError: not open
    f.do("resume", 1, snap)                                 # ValueError: open
    f.do("resume", 2, snap)
    f.do("set_embedding", 2, f.embed())
    f.feed()
    f.step()
    f.do("resume", 0, snap)
    f.do("close", 0)                                        # resumed and closed before a step: nothing is restored
    f.step()
    # many at once: a batch, the batch in place, a subset of its views, single snapshots stacked
    f.do("suspend_many", [1, 1])                            # ValueError: named twice
    batch = f.do("suspend_many", [2, 1])
    f.step()
    f.do("resume_many", [0, 1, 2], batch)                   # ValueError: 3 slots for 2 snapshots
    f.do("resume_many", [0, 1], batch)
    f.do("set_embedding", 1, f.embed())
    f.feed()
    f.step()
    f.do("open", 2, f.embed())
    f.step()
    slots, batch2 = f.do("drain")
    f.step()
    f.do("resume_many", [2, 0], [batch2[2], batch2[0]])
    f.do("resume_many", [1], [snap])
    f.do("resume_many", [], [])
    f.feed()
    f.step()
    f.get("rows_in_use")
    f.get("last_rows")
    # who is present
    if pace and not packets:
        for present in ([True, False, True], [True, False, True], [False, True, True], torch.tensor([True, True, False]),
                        None, [True, True]):
            f.step(present)
    else:
        f.step([True, False, True])                         # ValueError
    # packets of any size
    f.do("buffered", 0)
    f.do("ready")
    f.do("flush", 0)
    f.do("push", {0: f.packet(1)})
    if packets:
        f.do("push", {})
        f.do("push", {0: f.packet(0)})
        f.do("push", {0: f.packet(1), 1: f.packet(160)})
        f.do("push", {0: f.packet(320), 2: f.packet(333)})
        f.do("ready")
        for s in range(S):
            f.do("buffered", s)
        f.step()
        f.do("push", {1: f.packet(320)})
        f.do("push", {1: torch.zeros(3, 8)})                # ValueError
        f.step()
        f.do("flush", 0)                                    # no push behind it: the step issues one
        f.step()
        f.do("flush", 1)
        f.do("buffered", 1)
        f.do("push", {1: f.packet(160), 2: f.packet(333)})
        f.step()
        big = f.packet(333 * ss.client_rate // 16000)
        for _ in range(8):                                  # until the FIFO refuses: BufferError, nothing changed
            f.do("push", {0: f.packet(1), 2: big})
        for s in range(S):
            f.do("buffered", s)
        while f.do("ready"):
            f.step()
        f.do("step", torch.zeros(S, 2, 192))                # ValueError
    else:
        f.do("step")                                        # ValueError
    # the mix
    f.do("mix_of", 0)
    f.do("set_mix", 0, 0.5, 0.25)
    f.do("set_mix", 1, 2.0, 0.0)                            # ValueError
    f.do("mix_of", 0)
    f.feed()
    f.step()
    f.do("set_mix", 0, 0.5, 0.25)                           # the same targets: nothing travels
    f.step()
    # enrollment: to completion, to an abort, cancelled, while the embedder runs, with the room, on an open slot
    f.do("close", 1)
    f.do("enroll", 1, f.embedder)
    f.do("relook", 0, f.embedder)
    if enroll:
        done = ss._edone.numpy().view(np.uint32)                # the words the capture node posts
        f.do("enroll", 1, f.embedder)                       # ValueError: enrolling already
        f.do("open", 1, f.embed())                          # ValueError: enrolling
        f.get("enrolling")
        f.feed()
        f.step()
        f.step()
        done[1] = ss._capturing[1][0]                       # the clip is complete
        done[0] = ss._capturing[0][0]
        f.do("poll")
        f.get("enrolling")
        f.do("embedding_of", 1)
        f.do("embedding_of", 2)                             # ValueError
        f.feed()
        f.step()
        f.do("close", 1)
        f.do("enroll", 1, f.embedder)
        f.step()
        done[1] = ss._capturing[1][0] | FAULT               # a non-finite sample: the device aborts the capture
        f.do("faults")
        f.get("enrolling")
        f.do("open", 1, f.embed())                          # finds the slot idle: the poll of the shared check
        f.step()
        f.do("close", 1)
        f.do("enroll", 1, f.embedder)
        f.step()
        done[1] = ss._capturing[1][0] | FAULT
        f.do("resume", 1, snap)                             # the same through `resume`
        f.feed()
        f.step()
        f.do("close", 1)
        f.do("enroll", 1, f.embedder)
        f.step()
        f.do("close", 1)                                    # while capturing
        f.step()
        f.do("enroll", 1, f.embedder)
        f.step()
        done[1] = ss._capturing[1][0]
        ss._side.hold = True
        f.do("poll")
        f.get("enrolling")
        f.do("suspend", 1)                                  # ValueError: enrolling
        f.do("close", 1)                                    # while embedding: the result is dropped
        ss._side.hold = False
        f.feed()
        f.step()
        f.do("enroll", 1, f.embedder, passthrough=True)
        if monitor:
            f.do("mix_of", 1)
            f.step()
            f.step()
            done[1] = ss._capturing[1][0]
            f.step()
            f.do("mix_of", 1)
            f.step()
        else:
            f.do("enroll", 1, f.embedder)
            f.step()
        f.do("relook", 1, f.embedder)                       # open by now (monitor), or enrolling (ValueError)
        f.do("relook", 0, f.embedder)
        f.do("suspend", 0)                                  # ValueError: enrolling
        f.feed()
        f.step()
        done[0] = ss._capturing[0][0] if 0 in ss._capturing else 0
        f.step()
        f.do("embedding_of", 0)
        f.do("relook", 0, f.embedder)
        f.step()
        f.do("close", 0)                                    # cancels the look and closes the session
        f.step()
    # from the start again
    f.do("reset")
    f.get("active")
    f.feed()
    f.step()
    f.do("open", 2, f.embed())
    f.feed()
    f.step()
    f.do("_body", 0, S)                                     # what the emulator tests call


FLAVOURS = [
    ("plain", {}),
    ("compact", dict(compact=True)),
    ("pace", dict(pace=True)),
    ("pace+compact", dict(pace=True, compact=True)),
    ("enroll", dict(enroll_chunks=2)),
    ("pace+packets", dict(pace=True, packets=True, fifo_samples=512)),
    ("pace+packets+pcm16", dict(pace=True, packets=True, pcm16=True, fifo_samples=512)),
    ("pace+packets+48k", dict(pace=True, packets=True, client_rate=48000, fifo_samples=512)),
    ("pace+packets+48k+pcm16", dict(pace=True, packets=True, client_rate=48000, pcm16=True, fifo_samples=512)),
    ("pace+packets+compact+enroll+monitor", dict(pace=True, packets=True, compact=True, enroll_chunks=2, monitor=True,
                                                 fifo_samples=512)),
    ("enroll+monitor", dict(enroll_chunks=2, monitor=True)),
    ("compact+enroll", dict(compact=True, enroll_chunks=2)),
]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    tracer = Tracer()
    calls = lib = 0
    with open(args.out, "w") as out, tracer, torch.no_grad():
        net = make_net(tracer)
        for name, kw in FLAVOURS:
            f = Flavour(tracer, net, name, out, **kw)
            script(f)
            calls, lib = calls + f.n_calls, lib + f.n_lib
            print(f"{name}: {f.n_calls} public calls, {f.n_lib} library calls")
    print(f"total: {calls} public calls, {lib} library calls -> {args.out}")


if __name__ == "__main__":
    main()
