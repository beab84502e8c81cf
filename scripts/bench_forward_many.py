"""What `Net.forward_many` saves against `Net.forward` on the K-times-repeated mixtures, in DEVICE time per call (HIP events round
each call on the launch stream: the window streams fork from it and join it again, so the pair brackets the whole forward).

    python scripts/bench_forward_many.py [--out profiles/forward_many_cost.txt] [--shapes 1x3,4x3,8x4,11x3] [--seconds 5]
                                         [--steps 10] [--blocks 4] [--warmup 3]

Per shape B x K: `forward_many(x [B], embeds [B, K])` interleaved in ONE run with `forward(x repeated [B K], embeds [B K, 1])` on
inputs that are already on the device — blocks of `--steps` calls of each in turn, p50 over all calls; `scatter` is the spread of
the repeated-forward blocks' p50.  Both arms produce the same B K outputs.  Counted from the shapes, the shared form runs
(1 + 2 K) / 3 K of the block work of the three-block network; what it measures depends on which kernels and windows each
part takes at its batch, which the line of every shape names.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lookoncetohear_amd import config, synth  # noqa: E402
from lookoncetohear_amd.net import Net  # noqa: E402


def timed(fn, n, stream):
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", default="1x3,4x3,8x4,11x3")
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_forward_many.py measures on an MI355X; no device found (there is no CPU path)")
    dev = torch.device("cuda:0")
    net = Net(**config.TSH_PARAMS).eval()
    net.load_state_dict(config.separator_weights(0), strict=True)
    net = net.to(dev)
    stream = torch.cuda.current_stream(dev)
    n = int(args.seconds * synth.SR)
    T = -(-n // net.stft_chunk_size)
    lines = [f"forward_many against forward on the repeated mixtures: {args.seconds:g} s clips ({T} frames), device time per call, "
             f"{args.blocks} blocks of {args.steps} calls each, interleaved; {torch.cuda.get_device_properties(0).gcnArchName}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator().manual_seed(0)
    for shape in args.shapes.split(","):
        B, K = (int(v) for v in shape.split("x"))
        x = synth.batch(list(range(B)), n)["mixture"].to(dev)
        E = torch.nn.functional.normalize(torch.randn(B, K, 256, generator=g).abs(), dim=-1).to(dev)
        xr, Er = x.repeat_interleave(K, 0), E.reshape(B * K, 1, 256)
        arms = {"forward": lambda: net(xr, Er), "forward_many": lambda: net.forward_many(x, E)}
        with torch.no_grad():
            for fn in arms.values():
                timed(fn, args.warmup, stream)
            ms = {k: [] for k in arms}
            p50s = {k: [] for k in arms}
            for _ in range(args.blocks):
                for k, fn in arms.items():
                    blk = timed(fn, args.steps, stream)
                    ms[k] += blk
                    p50s[k].append(statistics.median(blk))
        if net.range_status(dev):
            raise SystemExit(f"B = {B}, K = {K}: non-finite samples")
        scatter = max(p50s["forward"]) - min(p50s["forward"])
        base, many = statistics.median(ms["forward"]), statistics.median(ms["forward_many"])
        mode = 1 if net.gemm_mode == "f16x3" else 0
        say(f"B = {B}, K = {K}: forward on {B * K} rows p50 {base:.3f} ms (min {min(ms['forward']):.3f}, max {max(ms['forward']):.3f}, "
            f"{net._n_time_chunks(B * K, T, mode)} windows), scatter of its blocks' p50 {1e3 * scatter:.1f} us")
        say(f"    forward_many: p50 {many:.3f} ms (min {min(ms['forward_many']):.3f}, max {max(ms['forward_many']):.3f}, blocks' p50 "
            f"spread {1e3 * (max(p50s['forward_many']) - min(p50s['forward_many'])):.1f} us; block 0 on {B} rows in "
            f"{net._n_time_chunks(B, T, mode)} windows) = {many / base:.3f} x forward, difference {1e3 * (many - base):+.1f} us: "
            f"{'WITHIN' if abs(many - base) <= 3 * scatter else 'BEYOND'} three times the scatter; "
            f"block work counted from the shapes {(1 + 2 * K) / (3 * K):.2f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
