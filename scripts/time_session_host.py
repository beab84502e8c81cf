"""Host time of `SessionStreamer.step()` and `push()`: what the calls cost the thread that makes them, enqueue only.

    python scripts/time_session_host.py [--against OTHER_NET_PY] [--device cuda:0|cpu] [--slots 1,64] [--out FILE]

The timed region is the call itself; nothing inside it synchronises, and the device is drained between blocks of 100 calls.
Per line `--blocks` blocks after 60 warm-up calls: the p50 of each block, then the median of those and their spread (max - min).
  steady: every slot open, nothing pending;  churn: one close and one open pending in every step (those two calls are outside
  the timed region, and so is a packet streamer's push);  push: one 128-sample packet for every slot, then an untimed step.
`--against FILE`: FILE is the `net.py` of another revision of this package that still defines `SessionStreamer`
(`git show REV:lookoncetohear_amd/net.py > FILE`).  It is loaded as a second module over the same `Net`, and blocks of the two
classes alternate in ONE process: two processes of the same code differ by more than the calls differ.  A line passes when
this tree's median is no more than three times the other revision's spread above the other revision's median.
`--device cpu` runs over a library stand-in that does nothing: the Python cost alone, on a machine without a GPU."""
import argparse
import contextlib
import importlib.util
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lookoncetohear_amd import config                                  # noqa: E402
from lookoncetohear_amd.net import Net                                 # noqa: E402
from lookoncetohear_amd.sessions import SessionStreamer                # noqa: E402

STEPS, WARM = 100, 60


class NullLib:
    def call(self, name, *args):
        pass

    def raw(self, name):
        return lambda *args: 0


class NullNet(Net):
    """`Net` over host tensors and a library that does nothing (the overrides of tests/hipemu/hosts.py)."""
    emu_lib = NullLib()

    def _lib(self, t):
        return self.emu_lib

    def _stream(self, device):
        return 0

    def _device_ctx(self, t):
        return contextlib.nullcontext()

    def _flag_words(self, device):
        return torch.zeros(2, dtype=torch.int32)

    def _host_words(self, n, device):
        return torch.zeros(n, dtype=torch.int32)

    def _enroll_side(self, dev):
        return None

    def _record_event(self, device):
        return None

    def _wait_event(self, device, ev, tensor=None):
        pass


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--against", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--slots", default="1,64")
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, cpu = args.device, args.device == "cpu"
    sync = (lambda: None) if cpu else torch.cuda.synchronize
    classes = {"this": SessionStreamer}
    if args.against:
        spec = importlib.util.spec_from_file_location("lookoncetohear_amd._net_other", args.against)
        other = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = other
        spec.loader.exec_module(other)
        classes = {"other": other.SessionStreamer, "this": SessionStreamer}
    net = (NullNet if cpu else Net)(**config.TSH_PARAMS).eval()
    if not cpu:
        net.load_state_dict(config.separator_weights(0), strict=True)
        net = net.to(dev)
    torch.manual_seed(0)
    rows = []
    for flavour, kw in (("plain", {}), ("pace+packets", dict(pace=True, packets=True))):
        for S in (int(s) for s in args.slots.split(",")):
            for what in ("steady", "churn") + (("push",) if kw else ()):
                emb = torch.randn(S, 256, device=dev)
                chunks = 0.1 * torch.randn(S, 2, 192, device=dev)
                packet = {s: 0.1 * torch.randn(2, 128) for s in range(S)}
                arms = {}
                for name, cls in classes.items():
                    ss = arms[name] = cls(net, S, dev, use_graph=not cpu, **kw)
                    for s in range(S):
                        ss.open(s, emb[s])
                    if kw:
                        ss.push({s: 0.1 * torch.randn(2, 64) for s in range(S)})     # the look-ahead, once

                def one(ss, i):
                    if what == "churn":
                        ss.close(i % S)
                        ss.open(i % S, emb[i % S])
                    if what == "push":
                        t0 = time.perf_counter()
                        ss.push(packet)
                        dt = time.perf_counter() - t0
                        ss.step()
                        return dt
                    if kw:
                        ss.push(packet)
                        t0 = time.perf_counter()
                        ss.step()
                    else:
                        t0 = time.perf_counter()
                        ss.step(chunks)
                    return time.perf_counter() - t0

                for ss in arms.values():
                    for i in range(WARM):
                        one(ss, i)
                sync()
                p50s = {name: [] for name in arms}
                for b in range(args.blocks):
                    for name, ss in arms.items():
                        lat = sorted(one(ss, b * STEPS + i) for i in range(STEPS))
                        sync()
                        p50s[name].append(lat[len(lat) // 2] * 1e6)
                row = dict(flavour=flavour, S=S, what=what)
                for name, v in p50s.items():
                    assert cpu or not arms[name].faults()
                    v.sort()
                    row[name + "_p50_us"], row[name + "_spread_us"] = round(v[len(v) // 2], 2), round(v[-1] - v[0], 2)
                line = f"{flavour:13s} S={S:<3d} {what:7s}" + "".join(
                    f"  {name} {row[name + '_p50_us']:7.2f} us (spread {row[name + '_spread_us']:5.2f})" for name in arms)
                if args.against:
                    row["diff_us"] = round(row["this_p50_us"] - row["other_p50_us"], 2)
                    row["within"] = row["diff_us"] <= 3 * row["other_spread_us"]
                    line += f"  this - other {row['diff_us']:+6.2f} us  {'within 3x' if row['within'] else 'NOT within 3x'}"
                rows.append(row)
                print(line, flush=True)
                del arms
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f)


if __name__ == "__main__":
    main()
