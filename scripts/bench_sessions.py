"""What the session layer costs per 8 ms chunk: `Streamer(B)` against `SessionStreamer(B)` with every slot open, same clip,
same loop and sync as `bench.py --mode stream`, in ONE process (the `Streamer` rows are the baseline: that class is what it
was before sessions existed).  Per batch size: Streamer, SessionStreamer, SessionStreamer with one close + one open every 25
chunks, Streamer again (drift of the box during the run).  Prints one JSON line; --out also writes it to a file.

    python scripts/bench_sessions.py [--batches 1,64] [--steps 625] [--warmup 100] [--out profiles/xyz.json]
    python scripts/bench_sessions.py --trace idle|reset --batches 8     # a short loop for rocprofv3 --kernel-trace --stats:
        idle = every slot open, nothing pending; reset = one close + one open pending in EVERY chunk
    python scripts/bench_sessions.py --enroll [--batches 1,64] [--enroll-chunks 625] [--out profiles/xyz.txt]
        what enrollment costs the chunk loop, in DEVICE time per chunk (HIP events around every replay on the loop's stream:
        `step` returns without waiting, a host timer would record the enqueue): (a) the capture node with nothing enrolling
        against a streamer built without it, interleaved in one run; (b) the chunks that overlap a running embedder call, one
        and four slots embedding, side stream at default and at lowest priority; (c) steps from the capture's last chunk to
        the slot's appearance in `active`.  The loop waits for every chunk's end event, as a real-time consumer does.
    python scripts/bench_sessions.py --compact [--slots 64] [--open 1,4,16,64] [--out profiles/xyz.txt]
        what row compaction buys and costs, in DEVICE time per chunk as above: (a) S slots with k listeners open, the lock-step
        streamer against the compacting one, blocks of the two interleaved in one run; `scatter` is the spread of the lock-step
        blocks' p50; (b) a step that moves one row and a step that moves eight, against the steps around them.
    python scripts/bench_sessions.py --pace [--batches 1,64] [--out profiles/xyz.txt]
        what pacing costs, in DEVICE time per chunk as above, the lock-step streamer and the paced one interleaved in one run:
        (a) every slot open and present, without a mask; (b) the largest batch with every second slot held; (c) the same with a
        mask that changes in every step, which is the path that copies the hold words.
    python scripts/bench_sessions.py --pace --trace idle|held --batches 64   # the short loop for rocprofv3, as above:
        idle = everyone present; held = every second slot held
    python scripts/bench_sessions.py --suspend [--batches 1,64] [--move-reps 20] [--out profiles/xyz.txt]
        what suspend / resume costs, in DEVICE time per chunk as above (the events enclose the call and the step it precedes), in
        a paced streamer with every slot open: a step that suspends one listener and, three steps later, a step that resumes
        them, against the steady steps of the same streamer in the same interleaved run; at the largest batch also the park
        and return of 8 listeners at once.  `scatter` is the spread of the steady blocks' p50.
    python scripts/bench_sessions.py --suspend-many [--slots 64] [--many 1,8,64] [--tiles 4,8,16,32] [--out profiles/xyz.txt]
        what the batched calls buy, in DEVICE time per chunk as above, in a paced streamer with every slot open.  Per k, one
        interleaved run of cycles: steady steps, a step that parks k listeners through `suspend_many`, 3 steps, a step that
        returns them through `resume_many`, steady steps, and the same two steps through the loops of `suspend` / `resume`.
        The batched step has to be cheaper than the loop by more than three times the scatter of the steady blocks.  --tiles:
        also the batched steps at the largest k under each tile count per (item, section) (lh_set_tuning key 18).
    python scripts/bench_sessions.py --packets [--batches 1,64] [--out profiles/packets_cost.txt]
        what the packet front costs, in DEVICE time per step as above (the events enclose `push` and the step it precedes, so
        the copy and the feed launch are counted), a packet-fed streamer against today's paced streamer, blocks of the two
        interleaved in one run: (a) every second slot alternately late, so presence changes in every step — 128-sample packets
        for the slots that are due against `step(chunks, present)` with the same mask, windows on the device and windows in
        pinned host memory; (b) everyone present.  The loop waits for every step, so the host's time inside `push` is in the
        interval; the `pipelined` arm enqueues the push for step i + 1 behind step i instead, as a host does that takes
        packets while the chunk runs.  `scatter` is the spread of the paced blocks' p50.
    python scripts/bench_sessions.py --client-rate 48000 [--batches 1,64] [--out profiles/client_rate_cost.txt]
        what resampling on the device costs a packet streamer, in DEVICE time per step, push included as above: everyone
        present, a chunk's worth of client samples per slot and step (384 at 48 kHz) against the 16 kHz packet streamer fed 128,
        blocks of the two interleaved in one run; `scatter` is the spread of the 16 kHz blocks' p50.  Then the offline
        `Resampler(client_rate, 16000)` on [64, 240000]: bytes read and written over the p50 time against the 8 TB/s of HBM.
    python scripts/bench_sessions.py --client-rate 44100 --any-rate [--batches 1,64] [--out profiles/any_rate_cost.txt]
        what the fractional hop costs, in DEVICE time per step, push included as above: everyone present, a step's worth of
        client samples per slot and step (352 or 353 at 44.1 kHz), the `any_rate=True` streamer against the 48 kHz streamer and
        the 16 kHz packet streamer, blocks of the three interleaved in one run; `scatter` is the spread of the 16 kHz blocks' p50.
    python scripts/bench_sessions.py --monitor [--batches 1,64] [--out profiles/monitor_cost.txt]
        what the monitor mix node costs, in DEVICE time per chunk as above, every slot open, the same streamer built with
        `monitor=False` and with `monitor=True`, blocks of the two interleaved in one run, in three states of the node: (a) settled
        at the defaults (the node returns after its loads), (b) both gains of every slot ramping through the whole block, (c)
        every slot settled at a mix of dry and wet.  `scatter` is the spread of the `monitor=False` blocks' p50; the bar for a
        difference is three times that.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lookoncetohear_amd import config, synth          # noqa: E402
from lookoncetohear_amd.net import Net                # noqa: E402

DEV = "cuda:0"


def timed(step, chunks, steps, warmup, before=None):
    n = len(chunks)
    for i in range(warmup):
        step(chunks[i % n])
    torch.cuda.synchronize()
    lat = []
    t0 = time.perf_counter()
    for i in range(steps):
        t1 = time.perf_counter()
        if before is not None:
            before(i)
        step(chunks[i % n])
        torch.cuda.synchronize()                 # a real-time consumer needs the chunk before the next one arrives
        lat.append(time.perf_counter() - t1)
    ms = (time.perf_counter() - t0) / steps * 1e3
    lat.sort()
    return {"ms_per_chunk": ms, "p50_ms": lat[len(lat) // 2] * 1e3, "p99_ms": lat[int(len(lat) * 0.99)] * 1e3,
            "max_ms": lat[-1] * 1e3}


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(len(v) * q))]


def dev_steps(ss, chunks, i0, n, before=None, until=None):
    """n steps (or until `until()` after a step) with events around each on the loop's stream -> [(start, end)] events."""
    evs = []
    for i in range(i0, i0 + n):
        if before is not None:
            before(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ss.step(chunks[i % len(chunks)])
        e1.record()
        e1.synchronize()
        evs.append((e0, e1))
        if until is not None and until():
            break
    return evs


def dev_steps_present(ss, chunks, n, present_of):
    """`dev_steps` of a paced streamer with the mask `present_of(i)` (None: no mask) -> ms per step."""
    ms = []
    for i in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ss.step(chunks[i % len(chunks)], present_of(i))
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    return {"n": len(ms), "p50_ms": pct(ms, 0.5), "p99_ms": pct(ms, 0.99), "max_ms": max(ms)}


def enroll_bench(net, args):
    from lookoncetohear_amd.embed_net import EmbedTFGridNet
    emb_net = EmbedTFGridNet(**config.EMBED_PARAMS).eval()
    emb_net.load_state_dict(config.embedder_weights(0), strict=True)
    emb_net = emb_net.to(DEV)
    n_en = args.enroll_chunks
    with torch.no_grad():
        for k in (1, 4):
            emb_net(torch.zeros(k, 2, 128 * n_en, device=DEV))       # packs the weights, fills the allocator's pools
    torch.cuda.synchronize()
    lines = [f"enrollment cost, device time per chunk (HIP events around each replay), enroll_chunks = {n_en}, "
             f"{args.steps} steps per block after {args.warmup} warm-up"]
    for B in [int(b) for b in args.batches.split(",")]:
        d = synth.batch(list(range(B)), 80000)
        mix = torch.nn.functional.pad(d["mixture"], (0, 64)).to(DEV)
        emb = d["embedding_gt"][:, 0].to(DEV)
        chunks = [mix[:, :, i * 128:i * 128 + 192].contiguous() for i in range(625)]
        # ---- (a) the capture node, nothing enrolling: blocks of the two streamers interleaved
        pair = {"without": net.make_session_streamer(B, DEV), "with": net.make_session_streamer(B, DEV, enroll_chunks=n_en)}
        ms = {k: [] for k in pair}
        for ss in pair.values():
            for s in range(B):
                ss.open(s, emb[s])
            dev_steps(ss, chunks, 0, args.warmup)
        for rep in range(4):
            for k, ss in pair.items():
                ms[k] += [a.elapsed_time(b) for a, b in dev_steps(ss, chunks, 0, args.steps // 4)]
        ra, rb = stats(ms["without"]), stats(ms["with"])
        lines.append(f"(a) S={B:3d} capture node idle   without: p50 {ra['p50_ms']:.4f} p99 {ra['p99_ms']:.4f} ms   with: p50 "
                     f"{rb['p50_ms']:.4f} p99 {rb['p99_ms']:.4f} ms   p50 cost {1e3 * (rb['p50_ms'] - ra['p50_ms']):+.1f} us")
        del pair
        # ---- (b), (c): k slots enroll at once (the others are open), at both priorities of the side stream
        for k in ([1] if B == 1 else [1, 4]):
            for low in (False, True):
                net.enroll_low_priority = low
                ss = net.make_session_streamer(B, DEV, enroll_chunks=n_en)
                net.enroll_low_priority = False
                for s in range(k, B):
                    ss.open(s, emb[s])
                dev_steps(ss, chunks, 0, args.warmup)
                spans = []

                def embedder(x):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    out = emb_net(x)
                    t1.record()
                    spans.append((t0, t1, x.shape[0]))
                    return out
                for s in range(k):
                    ss.enroll(s, embedder)
                evs = dev_steps(ss, chunks, 0, n_en)                 # the capture: its last chunk is evs[-1]
                base = [a.elapsed_time(b) for a, b in evs[n_en // 2:]]
                tail = dev_steps(ss, chunks, n_en, 2000, until=lambda: len(ss.active) == B)
                opened_after = len(tail)
                tail += dev_steps(ss, chunks, n_en + len(tail), 20)
                torch.cuda.synchronize()
                assert ss.faults() == [] and len(ss.active) == B and len(spans) == 1 and spans[0][2] == k
                ref = evs[0][0]
                t0, t1 = ref.elapsed_time(spans[0][0]), ref.elapsed_time(spans[0][1])
                over = [a.elapsed_time(b) for a, b in tail if ref.elapsed_time(b) > t0 and ref.elapsed_time(a) < t1]
                assert over, "no chunk overlapped the embedder call"
                ro, rn = stats(over), stats(base)
                worst = ro["max_ms"]
                lines.append(f"(b) S={B:3d} {k} embedding, side stream {'lowest ' if low else 'default'} priority: embedder "
                             f"{t1 - t0:.3f} ms, {ro['n']} chunks overlap it: p50 {ro['p50_ms']:.4f} p99 {ro['p99_ms']:.4f} max "
                             f"{ro['max_ms']:.4f} ms   (capturing, no embedder: p50 {rn['p50_ms']:.4f} p99 {rn['p99_ms']:.4f} max "
                             f"{rn['max_ms']:.4f} ms)   {'BELOW' if worst < 8.0 else 'NOT below'} the 8 ms chunk period")
                lines.append(f"(c) S={B:3d} {k} embedding, {'lowest ' if low else 'default'}: in `active` {opened_after} steps after the "
                             f"capture's last chunk (this loop runs chunks back to back; at one step per 8 ms: "
                             f"{1 + int((t1 - t0) // 8.0) + 1} steps)")
                del ss
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def compact_bench(net, args):
    S, reps = args.slots, 4
    d = synth.batch(list(range(S)), 80000)
    mix = torch.nn.functional.pad(d["mixture"], (0, 64)).to(DEV)
    emb = d["embedding_gt"][:, 0].to(DEV)
    chunks = [mix[:, :, i * 128:i * 128 + 192].contiguous() for i in range(625)]
    pair = {"lock-step": net.make_session_streamer(S, DEV), "compact": net.make_session_streamer(S, DEV, compact=True)}
    lines = [f"row compaction, device time per chunk (HIP events around each replay), S = {S}, buckets "
             f"{pair['compact'].row_buckets}, {args.steps} steps per figure in {reps} interleaved blocks after {args.warmup} warm-up"]
    # ---- (a) occupancy: k listeners open in both, blocks interleaved
    for k in [int(v) for v in args.open.split(",")]:
        ms, p50s = {n: [] for n in pair}, {n: [] for n in pair}
        for ss in pair.values():
            ss.reset()
            for s in range(k):
                ss.open(s, emb[s])
            dev_steps(ss, chunks, 0, args.warmup)
        for rep in range(reps):
            for n, ss in pair.items():
                blk = [a.elapsed_time(b) for a, b in dev_steps(ss, chunks, 0, args.steps // reps)]
                ms[n] += blk
                p50s[n].append(pct(blk, 0.5))
        torch.cuda.synchronize()
        assert all(ss.faults() == [] and len(ss.active) == k for ss in pair.values())
        rl, rc = stats(ms["lock-step"]), stats(ms["compact"])
        scatter = max(p50s["lock-step"]) - min(p50s["lock-step"])
        gain = rl["p50_ms"] - rc["p50_ms"]
        lines.append(f"(a) {k:3d} of {S} open, launched for {pair['compact'].last_rows:3d} rows   lock-step: p50 {rl['p50_ms']:.4f} p99 "
                     f"{rl['p99_ms']:.4f} ms   compact: p50 {rc['p50_ms']:.4f} p99 {rc['p99_ms']:.4f} ms   lock-step minus compact "
                     f"{1e3 * gain:+.1f} us, scatter of the lock-step blocks {1e3 * scatter:.1f} us: "
                     f"{'MORE' if gain > 3 * scatter else 'NOT more'} than three times the scatter")
    # ---- (b) the move step: all open, then the lowest m slots close in one step, so m rows move in its launch
    ss = pair["compact"]
    for m in (1, 8):
        if m >= S:
            continue
        quiet, moving = [], []
        for rep in range(args.move_reps):
            ss.reset()
            for s in range(S):
                ss.open(s, emb[s])
            evs = dev_steps(ss, chunks, 0, 12)
            quiet += [a.elapsed_time(b) for a, b in evs[4:]]
            for s in range(m):
                ss.close(s)
            (a, b), = dev_steps(ss, chunks, 12, 1)
            moving.append(a.elapsed_time(b))
            assert ss.rows_in_use == S - m
        rq, rm = stats(quiet), stats(moving)
        lines.append(f"(b) a step that moves {m} row{'s' if m > 1 else ' '} ({S} -> {S - m} listeners, {rm['n']} times): p50 "
                     f"{rm['p50_ms']:.4f} max {rm['max_ms']:.4f} ms   the steps before it: p50 {rq['p50_ms']:.4f} p99 "
                     f"{rq['p99_ms']:.4f} ms   p50 cost {1e3 * (rm['p50_ms'] - rq['p50_ms']):+.1f} us")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def pace_bench(net, args):
    reps = 4
    batches = [int(b) for b in args.batches.split(",")]
    lines = [f"pacing cost, device time per chunk (HIP events around each replay), {args.steps} steps per figure in {reps} "
             f"interleaved blocks after {args.warmup} warm-up; the yardstick is the lock-step SessionStreamer of the same run"]
    for B in batches:
        d = synth.batch(list(range(B)), 80000)
        mix = torch.nn.functional.pad(d["mixture"], (0, 64)).to(DEV)
        emb = d["embedding_gt"][:, 0].to(DEV)
        chunks = [mix[:, :, i * 128:i * 128 + 192].contiguous() for i in range(625)]
        lock, paced = net.make_session_streamer(B, DEV), net.make_session_streamer(B, DEV, pace=True)
        for ss in (lock, paced):
            for s in range(B):
                ss.open(s, emb[s])
        odd = [s % 2 == 0 for s in range(B)]
        if args.trace:                           # a short loop for rocprofv3 --kernel-trace --stats
            dev_steps_present(paced, chunks, 20, lambda i: None)         # everyone consumes a chunk first: no RESET is pending
            dev_steps_present(paced, chunks, 200, (lambda i: odd) if args.trace == "held" else (lambda i: None))
            continue
        dev_steps(lock, chunks, 0, args.warmup)
        dev_steps_present(paced, chunks, args.warmup, lambda i: None)
        flip = [odd, [not p for p in odd]]
        cases = [("(a) all present, no mask", lambda i: None)]
        if B == max(batches) and B > 1:
            cases += [("(b) every second slot held", lambda i: odd), ("(c) mask changes every step", lambda i: flip[i & 1])]
        for name, present_of in cases:
            ms, p50s = {"lock-step": [], "paced": []}, []
            for rep in range(reps):
                blk = [a.elapsed_time(b) for a, b in dev_steps(lock, chunks, 0, args.steps // reps)]
                ms["lock-step"] += blk
                p50s.append(pct(blk, 0.5))
                ms["paced"] += dev_steps_present(paced, chunks, args.steps // reps, present_of)
            torch.cuda.synchronize()
            assert lock.faults() == [] and paced.faults() == [] and len(paced.active) == B
            rl, rp = stats(ms["lock-step"]), stats(ms["paced"])
            cost = rp["p50_ms"] - rl["p50_ms"]
            lines.append(f"{name:30s} S={B:3d}   lock-step: p50 {rl['p50_ms']:.4f} p99 {rl['p99_ms']:.4f} ms   paced: p50 "
                         f"{rp['p50_ms']:.4f} p99 {rp['p99_ms']:.4f} ms   paced minus lock-step {1e3 * cost:+.1f} us "
                         f"({100.0 * cost / rl['p50_ms']:+.1f} %), scatter of the lock-step blocks "
                         f"{1e3 * (max(p50s) - min(p50s)):.1f} us")
        del lock, paced
    if args.trace:
        return
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def suspend_bench(net, args):
    def timed_step(ss, chunk, action=None):
        """One step in device time; `action` (the suspends or resumes of the step) is enqueued inside the interval."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if action is not None:
            action()
        ss.step(chunk)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    lines = [f"suspend / resume cost, device time per chunk (HIP events around the call and the replay), paced streamer, every "
             f"slot open, {args.move_reps} cycles of 12 steady steps, a step that suspends, 3 steps, a step that resumes"]
    batches = [int(b) for b in args.batches.split(",")]
    for B in batches:
        d = synth.batch(list(range(B)), 80000)
        mix = torch.nn.functional.pad(d["mixture"], (0, 64)).to(DEV)
        emb = d["embedding_gt"][:, 0].to(DEV)
        chunks = [mix[:, :, i * 128:i * 128 + 192].contiguous() for i in range(625)]
        ss = net.make_session_streamer(B, DEV, pace=True)
        for s in range(B):
            ss.open(s, emb[s])
        dev_steps(ss, chunks, 0, args.warmup)
        for m in ([1, 8] if B == max(batches) and B >= 8 else [1]):
            steady, p50s, park, back, i, snaps = [], [], [], [], 0, []
            for rep in range(args.move_reps):
                blk = [timed_step(ss, chunks[(i + j) % 625]) for j in range(12)][4:]
                steady += blk
                p50s.append(pct(blk, 0.5))
                park.append(timed_step(ss, chunks[(i + 12) % 625], lambda: snaps.extend(ss.suspend(s) for s in range(m))))
                for j in range(3):
                    timed_step(ss, chunks[(i + 13 + j) % 625])
                back.append(timed_step(ss, chunks[(i + 16) % 625], lambda: [ss.resume(s, snaps.pop(0)) for s in range(m)]))
                i += 17
            torch.cuda.synchronize()
            assert ss.faults() == [] and len(ss.active) == B and not snaps
            rs, scatter = stats(steady), max(p50s) - min(p50s)
            for name, ms in (("suspends", park), ("resumes", back)):
                r = stats(ms)
                cost = r["p50_ms"] - rs["p50_ms"]
                lines.append(f"S={B:3d} a step that {name} {m} listener{'s' if m > 1 else ' '} ({r['n']} times, "
                             f"{m * ss._snap_bytes / 1e6:.1f} MB of snapshots): p50 {r['p50_ms']:.4f} max {r['max_ms']:.4f} ms   "
                             f"steady steps: p50 {rs['p50_ms']:.4f} p99 {rs['p99_ms']:.4f} ms   p50 cost {1e3 * cost:+.1f} us, "
                             f"scatter of the steady blocks {1e3 * scatter:.1f} us: "
                             f"{'WITHIN' if cost <= 3 * scatter else 'NOT within'} three times the scatter")
        del ss
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def packets_bench(net, args):
    reps, N = 4, 80000
    lines = [f"packet front, device time per step (HIP events around push + step, or around step(chunks, present)), {args.steps} "
             f"steps per figure in {reps} interleaved blocks after {args.warmup} warm-up; the yardstick is the paced "
             f"SessionStreamer of the same run fed explicit windows"]
    for B in [int(b) for b in args.batches.split(",")]:
        d = synth.batch(list(range(B)), N)
        host = torch.nn.functional.pad(d["mixture"], (0, 64)).pin_memory()
        mix = host.to(DEV)
        emb = d["embedding_gt"][:, 0].to(DEV)
        chunks = [mix[:, :, i * 128:i * 128 + 192].contiguous() for i in range(625)]
        chunks_host = [host[:, :, i * 128:i * 128 + 192].contiguous().pin_memory() for i in range(625)]
        paced, fed = net.make_session_streamer(B, DEV, pace=True), net.make_session_streamer(B, DEV, pace=True, packets=True)
        for ss in (paced, fed):
            for s in range(B):
                ss.open(s, emb[s])
        even = [s % 2 == 0 for s in range(B)]
        flip = [even, [not p for p in even]]
        pos, push_us = [0] * B, []

        def next_packets(due):
            """The next 128 samples of every slot that is due, as a client sends them: a buffer of their own."""
            packets = {}
            for s, d in enumerate(due):
                if d:
                    packets[s] = host[s, :, pos[s]:pos[s] + 128].contiguous()
                    pos[s] = (pos[s] + 128) % N
            return packets

        def fed_steps(n, due_of, i0, pipelined=False):
            """n steps of the packet streamer; the slots of `due_of(i)` get their next 128 samples ahead of step i.  The packets
            exist before the interval starts.  Timed is push + step — or, `pipelined`, step i and then the push for step i + 1,
            which the host assembles while the device runs the chunk: `push` never waits."""
            ms = []
            if pipelined:
                fed.push(next_packets(due_of(i0)))
            for i in range(i0, i0 + n):
                ahead = pipelined and i + 1 < i0 + n
                packets = next_packets(due_of(i + 1)) if ahead else None if pipelined else next_packets(due_of(i))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                t0 = time.perf_counter()
                if not pipelined:
                    fed.push(packets)
                    push_us.append(1e6 * (time.perf_counter() - t0))
                fed.step()
                present = list(fed.last_present)
                if ahead:
                    fed.push(packets)
                e1.record()
                e1.synchronize()
                assert present == list(due_of(i)), i
                ms.append(e0.elapsed_time(e1))
            return ms

        def prime():
            """Every slot holds the 64 look-ahead samples: 128 more make a window, and a step leaves 64 again."""
            for s in range(B):
                fed.flush(s)
            fed.push({s: host[s, :, pos[s]:pos[s] + 64] for s in range(B)})
            for s in range(B):
                pos[s] += 64

        everyone = [True] * B
        arms = [("(a) presence changes every step", lambda i: flip[i & 1]), ("(b) everyone present", lambda i: everyone)]
        for name, due_of in arms:
            prime()
            i_fed = 0
            fed_steps(args.warmup, due_of, i_fed)
            i_fed += args.warmup
            mask_of = (lambda i: None) if due_of(0) is everyone else due_of
            dev_steps_present(paced, chunks, args.warmup, mask_of)
            ms, p50s = {"paced": [], "paced, host windows": [], "packets": [], "packets, pipelined": []}, []
            del push_us[:]
            for rep in range(reps):
                n = args.steps // reps
                blk = dev_steps_present(paced, chunks, n, mask_of)
                ms["paced"] += blk
                p50s.append(pct(blk, 0.5))
                ms["paced, host windows"] += dev_steps_present(paced, chunks_host, n, mask_of)
                ms["packets"] += fed_steps(n, due_of, i_fed)
                ms["packets, pipelined"] += fed_steps(n, due_of, i_fed + n, pipelined=True)
                i_fed += 2 * n
            torch.cuda.synchronize()
            assert paced.faults() == [] and fed.faults() == [] and len(fed.active) == B
            r = {k: stats(v) for k, v in ms.items()}
            scatter = max(p50s) - min(p50s)
            for k in ("paced, host windows", "packets", "packets, pipelined"):
                cost = r[k]["p50_ms"] - r["paced"]["p50_ms"]
                lines.append(f"{name:32s} S={B:3d}   paced, windows on the device: p50 {r['paced']['p50_ms']:.4f} p99 "
                             f"{r['paced']['p99_ms']:.4f} ms   {k}: p50 {r[k]['p50_ms']:.4f} p99 {r[k]['p99_ms']:.4f} ms   "
                             f"difference {1e3 * cost:+.1f} us ({100.0 * cost / r['paced']['p50_ms']:+.1f} %), scatter of the "
                             f"paced blocks {1e3 * scatter:.1f} us: {'WITHIN' if abs(cost) <= 3 * scatter else 'NOT within'} "
                             f"three times the scatter")
            cost = r["packets"]["p50_ms"] - r["paced, host windows"]["p50_ms"]
            lines.append(f"{name:32s} S={B:3d}   packets minus paced with host windows {1e3 * cost:+.1f} us; host time inside "
                         f"push (table, {sum(due_of(0))} or {sum(due_of(1))} packets, copy, launch): p50 {pct(push_us, 0.5):.1f} us")
        del paced, fed
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def client_rate_bench(net, args):
    from lookoncetohear_amd.resample import Resampler
    rate, reps, N, HBM = args.client_rate, 4, 80000, 8.0e12
    hop = 128 * rate // 16000
    lines = [f"client rate {rate} Hz, device time per step (HIP events around push + step), everyone present, {args.steps} steps per "
             f"figure in {reps} interleaved blocks after {args.warmup} warm-up; the yardstick is the 16 kHz packet streamer of the "
             f"same run"]
    for B in [int(b) for b in args.batches.split(",")]:
        d = synth.batch(list(range(B)), N)
        host16 = d["mixture"].pin_memory()
        # the same signal read at the client's rate: what is timed does not depend on the samples
        host_c = synth.batch(list(range(B)), N * rate // 16000)["mixture"].pin_memory() if rate != 16000 else host16
        emb = d["embedding_gt"][:, 0].to(DEV)
        base = net.make_session_streamer(B, DEV, pace=True, packets=True)
        cli = net.make_session_streamer(B, DEV, pace=True, packets=True, client_rate=rate)
        for ss in (base, cli):
            for s in range(B):
                ss.open(s, emb[s])

        def run(ss, host, per, n, pos):
            ms = []
            total = host.shape[-1]
            for _ in range(n):
                at = pos[0]
                packets = {s: host[s, :, at:at + per].contiguous() for s in range(B)}
                pos[0] = (at + per) % (total - per)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ss.push(packets)
                ss.step()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return ms

        pos16, posc = [0], [0]
        base.push({s: host16[s, :, :64] for s in range(B)})                  # the look-ahead, once
        cli.push({s: host_c[s, :, :64 * rate // 16000 + cli.lookahead_in] for s in range(B)})
        run(base, host16, 128, args.warmup, pos16), run(cli, host_c, hop, args.warmup, posc)
        assert all(base.last_present) and all(cli.last_present)
        ms, p50s = {"16 kHz": [], "client": []}, []
        for rep in range(reps):
            n = args.steps // reps
            blk = run(base, host16, 128, n, pos16)
            ms["16 kHz"] += blk
            p50s.append(pct(blk, 0.5))
            ms["client"] += run(cli, host_c, hop, n, posc)
            assert all(base.last_present) and all(cli.last_present)
        torch.cuda.synchronize()
        assert base.faults() == [] and cli.faults() == [] and len(cli.active) == B
        r = {k: stats(v) for k, v in ms.items()}
        scatter = max(p50s) - min(p50s)
        cost = r["client"]["p50_ms"] - r["16 kHz"]["p50_ms"]
        lines.append(f"S={B:3d}   16 kHz packets: p50 {r['16 kHz']['p50_ms']:.4f} p99 {r['16 kHz']['p99_ms']:.4f} ms   client rate {rate}: "
                     f"p50 {r['client']['p50_ms']:.4f} p99 {r['client']['p99_ms']:.4f} ms   difference {1e3 * cost:+.1f} us "
                     f"({100.0 * cost / r['16 kHz']['p50_ms']:+.1f} %), scatter of the 16 kHz blocks {1e3 * scatter:.1f} us: "
                     f"{'WITHIN' if abs(cost) <= 3 * scatter else 'NOT within'} three times the scatter")
        del base, cli
    rows, n_in = 64, 240000
    rs = Resampler(rate, 16000)
    x = torch.randn(rows, n_in, device=DEV)
    for _ in range(10):
        y = rs(x)
    ms = []
    for _ in range(50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = rs(x)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    moved = 4 * (x.numel() + y.numel())
    p50 = pct(ms, 0.5)
    lines.append(f"Resampler({rate}, 16000) on [{rows}, {n_in}] -> {list(y.shape)}: p50 {p50:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}, "
                 f"50 launches), {moved / 1e6:.1f} MB read + written = {moved / p50 * 1e3 / 1e12:.3f} TB/s = "
                 f"{moved / p50 * 1e3 / HBM:.3f} of HBM (8 TB/s)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def any_rate_bench(net, args):
    """`--client-rate 44100 --any-rate`: the fractional-hop streamer against the 48 kHz streamer and the 16 kHz packet streamer,
    blocks of the three interleaved in one run."""
    rate, reps, N = args.client_rate, 4, 80000
    lines = [f"any rate, client rate {rate} Hz (any_rate=True), device time per step (HIP events around push + step), everyone "
             f"present, {args.steps} steps per figure in {reps} interleaved blocks after {args.warmup} warm-up; the yardsticks are the "
             f"16 kHz packet streamer and the 48 kHz streamer of the same run; the bar for a difference is three times the scatter of "
             f"the 16 kHz blocks' p50"]
    for B in [int(b) for b in args.batches.split(",")]:
        emb = synth.batch(list(range(B)), N)["embedding_gt"][:, 0].to(DEV)
        mk = net.make_session_streamer
        arms = {"16 kHz": (mk(B, DEV, pace=True, packets=True), 16000),
                "48 kHz": (mk(B, DEV, pace=True, packets=True, client_rate=48000), 48000),
                f"{rate} Hz": (mk(B, DEV, pace=True, packets=True, client_rate=rate, any_rate=True), rate)}
        # the same kind of signal read at each rate: what is timed does not depend on the samples
        hosts = {k: synth.batch(list(range(B)), N * r // 16000)["mixture"].pin_memory() for k, (_, r) in arms.items()}
        pos, step_no = {k: 0 for k in arms}, {k: 0 for k in arms}
        for k, (ss, r) in arms.items():
            for s in range(B):
                ss.open(s, emb[s])
            # the look-ahead of the window and of the resampler, and one input block of slack: a step's samples arrive as
            # floor((i + 1) 128 r / 16000) - floor(i 128 r / 16000), while the 16 kHz side is made in whole blocks
            first = 64 * r // 16000 + (ss.lookahead_in + ss._o_in if r != 16000 else 0)
            ss.push({s: hosts[k][s, :, :first] for s in range(B)})
            pos[k] = first

        def run(k, n):
            (ss, r), host, ms = arms[k], hosts[k], []
            for _ in range(n):
                i = step_no[k]
                per = 128 * (i + 1) * r // 16000 - 128 * i * r // 16000
                step_no[k] = i + 1
                at = pos[k] if pos[k] + per <= host.shape[-1] else 0
                packets = {s: host[s, :, at:at + per].contiguous() for s in range(B)}
                pos[k] = at + per
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ss.push(packets)
                ss.step()
                e1.record()
                e1.synchronize()
                assert all(ss.last_present), (k, i)
                ms.append(e0.elapsed_time(e1))
            return ms

        for k in arms:
            run(k, args.warmup)
        ms, p50s = {k: [] for k in arms}, []
        for rep in range(reps):
            for k in arms:
                blk = run(k, args.steps // reps)
                ms[k] += blk
                if k == "16 kHz":
                    p50s.append(pct(blk, 0.5))
        torch.cuda.synchronize()
        assert all(ss.faults() == [] and len(ss.active) == B for ss, _ in arms.values())
        r = {k: stats(v) for k, v in ms.items()}
        scatter = max(p50s) - min(p50s)
        name = f"{rate} Hz"
        lines.append(f"S={B:3d}   " + "   ".join(f"{k}: p50 {r[k]['p50_ms']:.4f} p99 {r[k]['p99_ms']:.4f} ms" for k in arms))
        for k in ("16 kHz", "48 kHz"):
            cost = r[name]["p50_ms"] - r[k]["p50_ms"]
            lines.append(f"S={B:3d}   {name} minus {k}: {1e3 * cost:+.1f} us ({100.0 * cost / r[k]['p50_ms']:+.1f} %), scatter of the "
                         f"16 kHz blocks {1e3 * scatter:.1f} us: {'WITHIN' if abs(cost) <= 3 * scatter else 'NOT within'} three times "
                         f"the scatter")
        del arms
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def monitor_bench(net, args):
    reps = 4
    lines = [f"monitor mix cost, device time per chunk (HIP events around each replay), every slot open, {args.steps} steps per "
             f"figure in {reps} interleaved blocks after {args.warmup} warm-up; the yardstick is the SessionStreamer built with "
             f"monitor=False in the same run; the bar for a difference is three times the scatter of its blocks' p50"]
    never = 128 * 4 * (args.steps + args.warmup)           # a ramp that outlasts every step of state (b)
    for B in [int(b) for b in args.batches.split(",")]:
        d = synth.batch(list(range(B)), 80000)
        mix = torch.nn.functional.pad(d["mixture"], (0, 64)).to(DEV)
        emb = d["embedding_gt"][:, 0].to(DEV)
        chunks = [mix[:, :, i * 128:i * 128 + 192].contiguous() for i in range(625)]
        mk = net.make_session_streamer
        off = mk(B, DEV)
        states = [("(a) settled at the defaults", mk(B, DEV, monitor=True), None),
                  ("(b) every slot ramping", mk(B, DEV, monitor=True, monitor_ramp=never), (0.0, 1.0)),
                  ("(c) every slot dry + wet", mk(B, DEV, monitor=True, monitor_ramp=1), (0.7, 0.3))]
        for ss in [off] + [st[1] for st in states]:
            for s in range(B):
                ss.open(s, emb[s])
        dev_steps(off, chunks, 0, args.warmup)
        for name, on, target in states:
            if target is not None:
                for s in range(B):
                    on.set_mix(s, *target)
            dev_steps(on, chunks, 0, args.warmup)
            ms, p50s = {"off": [], "on": []}, []
            for rep in range(reps):
                blk = [a.elapsed_time(b) for a, b in dev_steps(off, chunks, 0, args.steps // reps)]
                ms["off"] += blk
                p50s.append(pct(blk, 0.5))
                ms["on"] += [a.elapsed_time(b) for a, b in dev_steps(on, chunks, 0, args.steps // reps)]
            torch.cuda.synchronize()
            assert off.faults() == [] and on.faults() == [] and len(on.active) == B
            gains = on._mix[1].cpu()
            if target is None:
                assert gains.tolist() == [[1.0] * B, [0.0] * B]
            elif on.monitor_ramp == never:
                assert (gains[0] > 0).all() and (gains[1] < 1).all(), "the ramp ended inside the measurement"
            ro, rn = stats(ms["off"]), stats(ms["on"])
            cost, scatter = rn["p50_ms"] - ro["p50_ms"], max(p50s) - min(p50s)
            lines.append(f"{name:30s} S={B:3d}   monitor=False: p50 {ro['p50_ms']:.4f} p99 {ro['p99_ms']:.4f} ms   monitor=True: p50 "
                         f"{rn['p50_ms']:.4f} p99 {rn['p99_ms']:.4f} ms   difference {1e3 * cost:+.1f} us "
                         f"({100.0 * cost / ro['p50_ms']:+.1f} %), scatter of the monitor=False blocks {1e3 * scatter:.1f} us: "
                         f"{'WITHIN' if abs(cost) <= 3 * scatter else 'NOT within'} three times the scatter")
        del off, states
    lines.append("for scale, the per-node figures README.md gives (rocprofv3 averages, B = 1 / 64): k_session_begin 2.4 / 6.3 us, "
                 "k_session_end 6.0 / 7.5 us; k_session_capture, the node of this one's shape (one wave per slot, one float4 per "
                 "lane), has no figure there yet")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def suspend_many_bench(net, args):
    from lookoncetohear_amd import _cabi

    def timed_step(ss, chunk, action=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if action is not None:
            action()
        ss.step(chunk)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    B = args.slots
    lines = [f"suspend_many / resume_many against the loops of suspend / resume, device time per chunk (HIP events around the calls "
             f"and the replay), paced streamer, S = {B}, every slot open, {args.move_reps} cycles of: 12 steady steps, a step that "
             f"parks k, 3 steps, a step that returns k — batched, then the same one by one"]
    d = synth.batch(list(range(B)), 80000)
    mix = torch.nn.functional.pad(d["mixture"], (0, 64)).to(DEV)
    emb = d["embedding_gt"][:, 0].to(DEV)
    chunks = [mix[:, :, i * 128:i * 128 + 192].contiguous() for i in range(625)]
    ss = net.make_session_streamer(B, DEV, pace=True)
    for s in range(B):
        ss.open(s, emb[s])
    dev_steps(ss, chunks, 0, args.warmup)
    held = []
    ways = {"suspend_many": lambda k: held.append(ss.suspend_many(range(k))),
            "resume_many": lambda k: ss.resume_many(range(k), held.pop()),
            "suspend loop": lambda k: held.append([ss.suspend(s) for s in range(k)]),
            "resume loop": lambda k: [ss.resume(s, snap) for s, snap in enumerate(held.pop())]}

    def cycles(k, pairs, reps):
        """-> (steady steps, p50 of each steady block, {way: ms of its steps})"""
        steady, p50s, ms, i = [], [], {w: [] for pair in pairs for w in pair}, 0
        for rep in range(reps):
            for park, back in pairs:
                blk = [timed_step(ss, chunks[(i + j) % 625]) for j in range(12)][4:]
                steady += blk
                p50s.append(pct(blk, 0.5))
                ms[park].append(timed_step(ss, chunks[(i + 12) % 625], lambda: ways[park](k)))
                for j in range(3):
                    timed_step(ss, chunks[(i + 13 + j) % 625])
                ms[back].append(timed_step(ss, chunks[(i + 16) % 625], lambda: ways[back](k)))
                i += 17
        torch.cuda.synchronize()
        assert ss.faults() == [] and len(ss.active) == B and not held
        return steady, p50s, ms

    ks = [int(k) for k in args.many.split(",")]
    for k in ks:
        steady, p50s, ms = cycles(k, (("suspend_many", "resume_many"), ("suspend loop", "resume loop")), args.move_reps)
        rs, scatter = stats(steady), max(p50s) - min(p50s)
        r = {w: stats(v) for w, v in ms.items()}
        for w in ms:
            lines.append(f"S={B:3d} k={k:2d} {w:13s} ({r[w]['n']} times, {k * ss._snap_bytes / 1e6:.1f} MB): p50 {r[w]['p50_ms']:.4f} "
                         f"max {r[w]['max_ms']:.4f} ms   steady steps: p50 {rs['p50_ms']:.4f} p99 {rs['p99_ms']:.4f} ms   "
                         f"p50 cost {1e3 * (r[w]['p50_ms'] - rs['p50_ms']):+.1f} us, scatter of the steady blocks {1e3 * scatter:.1f} us")
        for many, loop in (("suspend_many", "suspend loop"), ("resume_many", "resume loop")):
            gain = r[loop]["p50_ms"] - r[many]["p50_ms"]
            lines.append(f"S={B:3d} k={k:2d} {many} is {1e3 * gain:+.1f} us cheaper than the loop (p50): "
                         f"{'MORE than' if gain > 3 * scatter else 'NOT more than'} three times the scatter ({1e3 * scatter:.1f} us)")
        if k == B:
            lines.append(f"S={B:3d} k={k:2d} the step that returns everyone, chunk included: p50 {r['resume_many']['p50_ms']:.4f} max "
                         f"{r['resume_many']['max_ms']:.4f} ms batched, p50 {r['resume loop']['p50_ms']:.4f} max "
                         f"{r['resume loop']['max_ms']:.4f} ms one by one, against the 8 ms chunk period")
    if args.tiles:
        lib, k = _cabi.load(), max(ks)
        for t in [int(t) for t in args.tiles.split(",")]:
            lib.call("lh_set_tuning", 18, t)
            steady, p50s, ms = cycles(k, (("suspend_many", "resume_many"),), max(4, args.move_reps // 2))
            rs = stats(steady)
            lines.append(f"S={B:3d} k={k:2d} {t:3d} tiles per (item, section): " + "   ".join(
                f"{w} p50 {stats(v)['p50_ms']:.4f} max {max(v):.4f} ms (cost {1e3 * (stats(v)['p50_ms'] - rs['p50_ms']):+.1f} us)"
                for w, v in ms.items()) + f"   scatter {1e3 * (max(p50s) - min(p50s)):.1f} us")
        lib.call("lh_set_tuning", 18, 0)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--enroll", action="store_true")
    ap.add_argument("--pace", action="store_true")
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--suspend", action="store_true")
    ap.add_argument("--suspend-many", action="store_true")
    ap.add_argument("--packets", action="store_true")
    ap.add_argument("--client-rate", type=int, default=0)
    ap.add_argument("--any-rate", action="store_true")
    ap.add_argument("--monitor", action="store_true")
    ap.add_argument("--many", default="1,8,64")
    ap.add_argument("--tiles", default="")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--open", default="1,4,16,64")
    ap.add_argument("--move-reps", type=int, default=20)
    ap.add_argument("--enroll-chunks", type=int, default=625)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--steps", type=int, default=625)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--churn-every", type=int, default=25)
    ap.add_argument("--trace", choices=["idle", "reset", "held"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    net = Net(**config.TSH_PARAMS).eval()
    net.load_state_dict(config.separator_weights(0), strict=True)
    net = net.to(DEV)
    if args.enroll:
        return enroll_bench(net, args)
    if args.compact:
        return compact_bench(net, args)
    if args.pace:
        return pace_bench(net, args)
    if args.suspend:
        return suspend_bench(net, args)
    if args.suspend_many:
        return suspend_many_bench(net, args)
    if args.packets:
        return packets_bench(net, args)
    if args.client_rate and args.any_rate:
        return any_rate_bench(net, args)
    if args.client_rate:
        return client_rate_bench(net, args)
    if args.monitor:
        return monitor_bench(net, args)
    rows = []
    for B in [int(b) for b in args.batches.split(",")]:
        d = synth.batch(list(range(B)), 80000)
        mix = torch.nn.functional.pad(d["mixture"], (0, 64)).to(DEV)
        emb = d["embedding_gt"][:, 0].to(DEV)
        chunks = [mix[:, :, i * 128:i * 128 + 192].contiguous() for i in range(625)]
        ss = net.make_session_streamer(B, DEV)
        for s in range(B):
            ss.open(s, emb[s])

        def churn(i, every=args.churn_every):
            if i % every == 0:
                slot = (i // every) % B
                ss.close(slot)
                ss.open(slot, emb[slot])
        if args.trace:
            timed(ss.step, chunks, 200, 20, before=(lambda i: churn(i, 1)) if args.trace == "reset" else None)
            continue
        st = net.make_streamer(B, DEV)
        st.set_embedding(emb)
        r = {"batch": B, "steps": args.steps, "warmup": args.warmup}
        r["streamer"] = timed(st.step, chunks, args.steps, args.warmup)
        r["sessions"] = timed(ss.step, chunks, args.steps, args.warmup)
        r["sessions_churn"] = timed(ss.step, chunks, args.steps, args.warmup, before=churn)
        r["streamer_again"] = timed(st.step, chunks, args.steps, args.warmup)
        assert ss.faults() == [] and len(ss.active) == B
        base = min(r["streamer"]["p50_ms"], r["streamer_again"]["p50_ms"])
        r["extra_p50_pct"] = 100.0 * (r["sessions"]["p50_ms"] / base - 1.0)
        r["extra_p50_pct_churn"] = 100.0 * (r["sessions_churn"]["p50_ms"] / base - 1.0)
        r["baseline_spread_pct"] = 100.0 * (r["streamer"]["p99_ms"] / r["streamer"]["p50_ms"] - 1.0)
        rows.append(r)
        del st, ss
    if args.trace:
        return
    line = json.dumps({"metric": "chunk latency, Streamer vs SessionStreamer (all slots open), graph replay", "unit": "ms",
                       "churn_every": args.churn_every, "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
