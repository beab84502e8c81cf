"""What a chunk of m frames costs: `Streamer(B, frames_per_chunk=m)` for B in --batches and m in --frames, every streamer
built once and their blocks interleaved in ONE process, so the m = 1 streamer of the same run is the baseline (never a figure
from a document).

    python scripts/bench_stream_frames.py [--batches 1,64] [--frames 1,2,4,8,16] [--steps 600] [--blocks 10] [--warmup 50]
                                          [--out profiles/stream_frames_cost.txt]
        DEVICE time per `step`, input copy included: HIP events on the loop's stream around every `step` (which returns
        without waiting: a host timer would record the enqueue); the loop waits for every step's end event, as a real-time
        consumer does.  Per configuration p50 and p99 of --steps steps taken in --blocks blocks; one round of the run is one
        block of every configuration.  `scatter` per batch size = half the p10..p90 range of the m = 1 blocks' p50; a
        difference is claimed only beyond three times the scatter.  Per configuration: ms per step, ms per 8 ms frame
        (step / m), the difference of that to m = 1 with its verdict, and real-time streams per GPU at RTF 0.5 =
        B * 0.5 * 8 m / step_ms.
    python scripts/bench_stream_frames.py --trace 64,8      # a short loop of one configuration for rocprofv3 --kernel-trace --stats
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lookoncetohear_amd import config, synth          # noqa: E402
from lookoncetohear_amd.net import Net                # noqa: E402

DEV = "cuda:0"
HOP, LOOK, FRAMES = 128, 64, 624          # frames of the clip the chunks are cut from: a multiple of 1, 2, 4, 8 and 16


def chunks_of(mix, m):
    return [mix[:, :, i * HOP * m:(i + 1) * HOP * m + LOOK].contiguous() for i in range(FRAMES // m)]


def dev_steps(st, chunks, i0, n):
    """n steps with events around each on the loop's stream -> ms per step."""
    ms = []
    for i in range(i0, i0 + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st.step(chunks[i % len(chunks)])
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--frames", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--trace", default=None, help="B,m: a short loop of that configuration only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_frames.py measures on the GPU; none found")
    net = Net(**config.TSH_PARAMS).eval()
    net.load_state_dict(config.separator_weights(0), strict=True)
    net = net.to(DEV)
    batches = [int(b) for b in args.batches.split(",")]
    frames = [int(m) for m in args.frames.split(",")]
    if args.trace:
        B, m = (int(v) for v in args.trace.split(","))
        batches, frames = [B], [m]
    elif 1 not in frames:
        raise SystemExit("--frames must contain 1: the m = 1 streamer of the same run is the baseline")

    cfgs = {}
    for B in batches:
        d = synth.batch(list(range(B)), HOP * FRAMES + LOOK)
        mix, emb = d["mixture"].to(DEV), d["embedding_gt"][:, 0].to(DEV)
        for m in frames:
            st = net.make_streamer(B, DEV, use_graph=True, frames_per_chunk=m)
            st.set_embedding(emb)
            cfgs[B, m] = (st, chunks_of(mix, m))
    if args.trace:
        st, chunks = cfgs[batches[0], frames[0]]
        dev_steps(st, chunks, 0, 220)
        torch.cuda.synchronize()
        return

    for st, chunks in cfgs.values():
        dev_steps(st, chunks, 0, args.warmup)
    per = max(1, args.steps // args.blocks)
    ms = {k: [] for k in cfgs}
    p50s = {k: [] for k in cfgs}
    for blk in range(args.blocks):
        for k, (st, chunks) in cfgs.items():
            b = dev_steps(st, chunks, args.warmup + blk * per, per)
            ms[k] += b
            p50s[k].append(float(np.percentile(b, 50)))
    torch.cuda.synchronize()
    for (B, m), (st, _) in cfgs.items():
        assert int(st.range_flag[0]) == 0 and bool(torch.isfinite(st.out).all()), (B, m)

    lines = [f"Streamer(B, frames_per_chunk=m): device time per step (HIP events around each step, input copy included, graph "
             f"replay), {per * args.blocks} steps per configuration in {args.blocks} blocks, one block of every configuration per "
             f"round, after {args.warmup} warm-up steps each; baseline = the m = 1 streamer of this run; scatter = half the "
             f"p10..p90 range of the m = 1 blocks' p50; a difference in ms per frame is claimed beyond 3 x scatter",
             f"{'B':>3s} {'m':>3s} {'latency ms':>10s} {'step p50 ms':>12s} {'p99 ms':>8s} {'ms / frame':>11s} {'vs m=1 us':>10s} "
             f"{'streams at RTF 0.5':>19s}  verdict"]
    for B in batches:
        base = float(np.percentile(ms[B, 1], 50))
        sc = float(np.percentile(p50s[B, 1], 90) - np.percentile(p50s[B, 1], 10)) / 2
        lines.append(f"B = {B}: m = 1 step p50 {base:.4f} ms, scatter {1e3 * sc:.2f} us")
        for m in frames:
            p50, p99 = float(np.percentile(ms[B, m], 50)), float(np.percentile(ms[B, m], 99))
            pf = p50 / m
            dlt = pf - base
            verdict = "baseline" if m == 1 else ("cheaper per frame" if dlt < -3 * sc else
                                                 "NOT cheaper per frame: dearer" if dlt > 3 * sc else
                                                 "NOT cheaper per frame: within 3 x scatter")
            lines.append(f"{B:3d} {m:3d} {8 * m + 4:10d} {p50:12.4f} {p99:8.4f} {pf:11.4f} {1e3 * dlt:+10.1f} "
                         f"{B * 0.5 * 8 * m / p50:19.0f}  {verdict}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
