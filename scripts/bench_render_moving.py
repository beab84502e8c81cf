"""What rendering MOVING sources costs against the static renderer, in DEVICE time per call (HIP events round each call on the
launch stream; the entry points are called through the C ABI on preallocated buffers, so no host read sits between the events).

    python scripts/bench_render_moving.py [--out profiles/render_moving_cost.txt] [--batch 32] [--rows 4] [--n 80000]
                                          [--lh 64,256,4096] [--steps 10] [--blocks 4] [--warmup 3] [--fft]

Per response length: `lh_render_moving` (frame 400, a bank of 72 entries per utterance) interleaved in ONE run with
`lh_render_binaural` on the same sources — blocks of `--steps` calls of each in turn, p50 per block; `scatter` is the spread of
the static blocks' p50.  Two kinds of path: `every frame` (consecutive path points always name different entries: two chains
in every frame) and `arcs` (synth's piecewise-arc law through `lh_path_nearest`: most frames rest and run one chain).  Lh = 64 and
256 are direct form on both sides; at Lh = 4096 the static call takes its overlap-save FFT path and the moving one stays direct.
`lh_path_nearest` is reported on its own (B x rows paths of 201 points against 1250 positions).  The operations are counted from
the shapes: 2 x N x Lh x 2 ears per row and chain.
`--fft` adds, in the SAME interleaved run, the partitioned overlap-save form `lh_render_moving_fft` on both kinds of path — with
the bank's spectra computed before (`cached image`) and with `lh_bank_spectra` inside the timed call (`image in the call`) — and
`lh_bank_spectra` alone; each is held against the direct moving call and the static call of that run
(profiles/render_moving_fft_cost.txt: --fft --lh 256,512,1024,2048,4096,8192).
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lookoncetohear_amd import _cabi, synth  # noqa: E402

FRAME, P, K = 400, 72, 4


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--n", type=int, default=80000)
    ap.add_argument("--lh", default="64,256,4096")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fft", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_moving.py measures on an MI355X; no device found (there is no CPU path)")
    dev = torch.device("cuda:0")
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    B, S1, N = args.batch, args.rows, args.n
    F = -(-N // FRAME) + 1
    g = torch.Generator().manual_seed(0)
    D = lambda t: t.data_ptr()
    lines = [f"render_moving against render: B = {B}, S1 = {S1}, N = {N}, frame = {FRAME}, P = {P}, K = {K}; device time per call, "
             f"{args.blocks} blocks of {args.steps} calls each, interleaved; {torch.cuda.get_device_properties(0).gcnArchName}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    src = (0.1 * torch.randn(B, S1, N, generator=g)).to(dev)
    gain = (0.5 + torch.rand(B, S1, generator=g)).to(dev)
    tgt = torch.zeros(B, dtype=torch.int32, device=dev)
    bank_of = (torch.arange(B) % K).to(torch.int32).to(dev)
    ev = torch.empty(B, S1, 2, N, device=dev)
    mx, tg = torch.empty(B, 2, N, device=dev), torch.empty(B, 2, N, device=dev)
    pk = torch.empty(B, dtype=torch.int32, device=dev)

    # paths: every frame moving, and the piecewise-arc law looked up on the device
    every = ((torch.arange(F)[None, None] + torch.arange(S1)[None, :, None] * 7 + torch.arange(B)[:, None, None] * 3) % P).to(torch.int32).to(dev)
    az = 2 * np.pi * np.arange(P) / P
    ring = torch.from_numpy(np.stack([np.cos(az), np.sin(az), np.zeros(P)], 1).astype(np.float32))
    positions = ring[None].repeat(K, 1, 1).to(dev)
    rs = np.random.RandomState(0)
    a = np.stack([[synth._path_azimuths(rs, 1, F, FRAME / synth.SR) for _ in range(S1)] for _ in range(B)])
    paths = torch.from_numpy((1.5 * np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], -1)).astype(np.float32)).to(dev)
    arcs = torch.empty(B, S1, F, dtype=torch.int32, device=dev)
    lib.call("lh_path_nearest", D(paths), D(positions), D(bank_of), D(arcs), B, S1, F, P, K, st)
    torch.cuda.synchronize()
    used = arcs[:, :, :F]
    rest = float((used[:, :, 1:] == used[:, :, :-1]).float().mean())
    say(f"paths: `every frame` 0 % resting frames; `arcs` {100 * rest:.1f} % resting frames (idx[f] == idx[f + 1])")

    for Lh in [int(v) for v in args.lh.split(",")]:
        bank = (torch.randn(K, P, 2, Lh, generator=g) / Lh ** 0.5).to(dev)
        rir = bank[bank_of.long()[:, None], every[:, :, 0].long()].contiguous()                    # [B][S1][2][Lh]
        static = lambda: lib.call("lh_render_binaural", D(src), D(rir), D(gain), D(tgt), D(ev), D(pk), D(mx), D(tg), B, S1, N, Lh, st)
        moving = lambda idx: (lambda: lib.call("lh_render_moving", D(src), D(bank), D(bank_of), D(idx), D(gain), D(tgt), D(ev), D(pk),
                                               D(mx), D(tg), B, S1, N, Lh, P, K, F, FRAME, st))
        arms = {"static": static, "moving, every frame": moving(every), "moving, arcs": moving(arcs)}
        if args.fft:
            from lookoncetohear_amd.render import FFT_LDS_RING, FFT_Z, fft_partition
            _, _, Q, ring, run = fft_partition(Lh, FRAME)
            spec = torch.empty(K, P, Q, FFT_Z, 2, device=dev)
            runs = -(-(-(-N // FRAME)) // run)
            work = torch.empty(B * S1 * runs * ring * FFT_Z, 2, device=dev) if ring > FFT_LDS_RING else None
            image = lambda: lib.call("lh_bank_spectra", D(bank), D(spec), K, P, Lh, FRAME, st)
            image()
            fft = lambda idx: (lambda: lib.call("lh_render_moving_fft", D(src), D(spec), D(bank_of), D(idx), D(gain), D(tgt), D(ev),
                                                D(pk), D(mx), D(tg), None if work is None else D(work), B, S1, N, Lh, P, K, F, FRAME, st))
            both = lambda idx: (lambda f=fft(idx): (image(), f()))
            arms.update({"fft, every frame, cached image": fft(every), "fft, arcs, cached image": fft(arcs),
                         "fft, every frame, image in the call": both(every), "fft, arcs, image in the call": both(arcs),
                         "lh_bank_spectra": image})
        for fn in arms.values():
            timed(fn, args.warmup, stream)
        ms = {k: [] for k in arms}
        p50s = {k: [] for k in arms}
        for _ in range(args.blocks):
            for k, fn in arms.items():
                blk = timed(fn, args.steps, stream)
                ms[k] += blk
                p50s[k].append(statistics.median(blk))
        scatter = max(p50s["static"]) - min(p50s["static"])
        base = statistics.median(ms["static"])
        path = "overlap-save FFT" if 1024 <= Lh <= 4097 else "direct form"
        flop = 2.0 * B * S1 * 2 * N * Lh
        say(f"Lh = {Lh}: static ({path}) p50 {base:.4f} ms (min {min(ms['static']):.4f}, max {max(ms['static']):.4f}), scatter of its "
            f"blocks' p50 {1e3 * scatter:.1f} us" + (f", {flop / base / 1e9:.1f} TFLOP/s" if path == "direct form" else ""))
        for k in ("moving, every frame", "moving, arcs"):
            p50 = statistics.median(ms[k])
            chains = 2.0 if k.endswith("frame") else 2.0 - rest
            say(f"    {k}: p50 {p50:.4f} ms (min {min(ms[k]):.4f}, max {max(ms[k]):.4f}, blocks' p50 spread "
                f"{1e3 * (max(p50s[k]) - min(p50s[k])):.1f} us) = {p50 / base:.2f} x static, difference {1e3 * (p50 - base):+.1f} us: "
                f"{'WITHIN' if abs(p50 - base) <= 3 * scatter else 'NOT within'} three times the scatter; "
                f"{chains * flop / p50 / 1e9:.1f} TFLOP/s over {chains:.2f} chains per output")
        if args.fft:
            say(f"    lh_bank_spectra ({K} x {P} entries x {Q} partitions, image {K * P * Q * FFT_Z * 8 / 2 ** 20:.1f} MiB"
                f"{'' if work is None else f', scratch {work.numel() * 4 / 2 ** 20:.0f} MiB'}): p50 "
                f"{statistics.median(ms['lh_bank_spectra']):.4f} ms")
            for kind in ("every frame", "arcs"):
                direct = statistics.median(ms[f"moving, {kind}"])
                for how in ("cached image", "image in the call"):
                    k = f"fft, {kind}, {how}"
                    p50 = statistics.median(ms[k])
                    say(f"    {k}: p50 {p50:.4f} ms (min {min(ms[k]):.4f}, max {max(ms[k]):.4f}, blocks' p50 spread "
                        f"{1e3 * (max(p50s[k]) - min(p50s[k])):.1f} us) = {p50 / base:.2f} x static, {direct / p50:.2f} x faster than "
                        f"the direct moving call ({1e3 * (direct - p50):+.1f} us): "
                        f"{'FASTER' if direct - p50 > 3 * scatter else 'NOT faster'} by more than three times the scatter")

    Pn, Fn = 1250, 201
    posn = torch.nn.functional.normalize(torch.randn(K, Pn, 3, generator=g), dim=-1).to(dev)
    pathn = (1.5 * torch.nn.functional.normalize(torch.randn(B, S1, Fn, 3, generator=g), dim=-1)).to(dev)
    outn = torch.empty(B, S1, Fn, dtype=torch.int32, device=dev)
    near = lambda: lib.call("lh_path_nearest", D(pathn), D(posn), D(bank_of), D(outn), B, S1, Fn, Pn, K, st)
    timed(near, args.warmup, stream)
    t = timed(near, args.steps * args.blocks, stream)
    say(f"lh_path_nearest, {B * S1 * Fn} points x {Pn} positions: p50 {1e3 * statistics.median(t):.1f} us (min {1e3 * min(t):.1f}, "
        f"max {1e3 * max(t):.1f})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
