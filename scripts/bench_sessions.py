"""What the session layer costs per 8 ms chunk: `Streamer(B)` against `SessionStreamer(B)` with every slot open, same clip,
same loop and sync as `bench.py --mode stream`, in ONE process (the `Streamer` rows are the baseline: that class is what it
was before sessions existed).  Per batch size: Streamer, SessionStreamer, SessionStreamer with one close + one open every 25
chunks, Streamer again (drift of the box during the run).  Prints one JSON line; --out also writes it to a file.

    python scripts/bench_sessions.py [--batches 1,64] [--steps 625] [--warmup 100] [--out profiles/xyz.json]
    python scripts/bench_sessions.py --trace idle|reset --batches 8     # a short loop for rocprofv3 --kernel-trace --stats:
        idle = every slot open, nothing pending; reset = one close + one open pending in EVERY chunk
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--steps", type=int, default=625)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--churn-every", type=int, default=25)
    ap.add_argument("--trace", choices=["idle", "reset"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    net = Net(**config.TSH_PARAMS).eval()
    net.load_state_dict(config.separator_weights(0), strict=True)
    net = net.to(DEV)
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
