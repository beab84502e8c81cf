"""Developer tool: which activation streams gain from the non-temporal cache policy (csrc/lh_cachepol.h)?

    python scripts/ab_policy.py build [MASK ...]       (no GPU) the one-bit libraries, or the given stream sets (0x...)
    python scripts/ab_policy.py run [--batch 32] [--rounds 40] [--group 4] [MASK ...]      (GPU)
    python scripts/ab_policy.py sweep [--rounds 12] [B ...]                                (GPU) the footprint threshold

`build` compiles, per variant, the two sources whose kernels carry a policy with -DLH_NT_MASK=<mask> and links them with the
product build's other objects (build.build_hip(only=...)): lookoncetohear_amd/_lookonce_hip_nt<mask>.so.
The nine streams are those of the three frame kernels.  profiles/cache_policy_ab.txt also has rows for nine more (the rows of
the two recurrences, the front end's store, the back end's load): those came from a lab patch of those kernels and of this
script that is not kept, because none of them moved — this script cannot reproduce them.
`run` loads the product library (lh_set_tuning(19, 0): plain accesses) and every variant (19 = 2: policy forced on) into ONE
process and times each C-ABI stage call of a block at the given batch on real workspaces (5 s clips, filled by a forward of the
stages), the libraries interleaved round-robin.  A HIP event pair brackets a GROUP of calls, not each call (a record costs
~6 us of stream time, profiles/r05q_ab_event_stride.txt).  Two kinds of group:
  * one stage, `--group` calls back to back: what the stage's own accesses cost it (only variants that touch the stage);
  * the chain of a forward's stages once (front end, a block, the closing stage in both forms, back end), with an event at
    every stage boundary: stores that evict and loads that stream interact across launches, so a set of bits is judged
    here (`in <stage>` rows: the stage's time with the cache in the state its predecessor left).
Per group: p50 per library, the baseline's scatter (half its p10..p90 range; the product library also runs a second time as
`A/A`, the null), and p50(variant) - p50(baseline).  A bit is kept if its stage gains more than three times that scatter.
Every variant's outputs are compared with the baseline's, bit for bit, before anything is timed.
`sweep`: whole forwards of the product library on 5 s clips (the harness of scripts/batch_sweep.py) per batch size, the policy
forced off and on (lh_set_tuning(19, 0 / 2)) in alternation; the threshold of csrc/lh_cachepol.h (NT_MIN_BYTES) is the smallest
footprint from which forced-on wins at every larger size."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lookoncetohear_amd import build  # noqa: E402

STREAMS = ["QKV_X_LD", "QKV_ST", "ATT_Q_LD", "ATT_K_LD", "ATT_V_LD", "ATT_MERGED_ST", "PROJ_MERGED_LD", "PROJ_RES_LD",
           "PROJ_ST"]                       # bit order of lh::cp::Stream
POLICY_SOURCES = ("lh_pointwise.hip", "lh_attn.hip")      # the sources whose kernels carry a policy
STAGE_BITS = {"fe": 0, "intra": 0, "inter": 0, "qkv": 0x3, "attn": 0x3c, "proj": 0x1c0, "taps": 0x1c0, "be": 0}


def names(mask):
    return "+".join(n for i, n in enumerate(STREAMS) if mask >> i & 1) or "plain"


def lib_path(mask):
    return os.path.join(build.PKG, f"_lookonce_hip_nt{mask:03x}.so")


def build_variant(mask):
    """Both policy sources are compiled with the variant's table every time (the product objects carry the committed table,
    and `run` forces the policy on: a source left at the product table would add its streams to the variant's)."""
    out = build.build_hip(force=True, verbose=False, extra_flags=[f"-DLH_NT_MASK={mask:#x}u"], out=lib_path(mask),
                          only=POLICY_SOURCES)
    print(f"{out}  {names(mask)}", flush=True)


def cmd_build(masks):
    build.build_hip()                        # the product objects the variants link against
    with ThreadPoolExecutor(max_workers=min(4, os.cpu_count() or 1)) as ex:
        list(ex.map(build_variant, masks))


def cmd_run(masks, batch, rounds, group):
    import numpy as np
    import torch
    from lookoncetohear_amd import _cabi, config, synth
    from lookoncetohear_amd.net import Net

    dev = torch.device("cuda", 0)
    net = Net(**config.TSH_PARAMS).eval()
    net.load_state_dict(config.separator_weights(0), strict=True)
    net = net.to(dev)
    d = synth.batch(list(range(8)), 80000)
    mix = d["mixture"].repeat((batch + 7) // 8, 1, 1)[:batch].contiguous().to(dev)
    B, T = batch, (mix.shape[-1] - net.nfft) // net.stft_chunk_size + 1
    ns = (T - 1) * net.stft_chunk_size + net.nfft
    mix = mix[..., :ns].contiguous()
    pk, ws = net._weights(dev), net._workspace(B, T, dev)
    bp = pk["blocks"][1 if net.n_blocks > 1 else 0]
    zs = net._zero_state(B, dev)
    bs = zs["gridnet_bufs"]["buf0"]
    st = torch.cuda.current_stream(dev).cuda_stream
    P = lambda t: t.data_ptr()
    E = lambda t: torch.empty_like(t)
    xa, xb, xc = ws["xa"], ws["xb"], ws["xc"]
    m, xo = E(xa), E(xa)                      # attention output / projection output: every stage keeps its own input intact
    ptaps, fmax = torch.empty(B * T * 97 * 36, device=dev), torch.empty(B * T, device=dev)
    y = torch.empty(B, net.n_srcs, net.stft_chunk_size * T, device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    h0, c0 = bs["h0"].contiguous().float(), bs["c0"].contiguous().float()
    hN, cN, conv_in = E(h0), E(c0), zs["conv_buf"].contiguous().float()
    conv_out = E(conv_in)
    ws["kx"][:, :net.local_atten_len - 1].zero_()
    ws["vx"][:, :net.local_atten_len - 1].zero_()

    calls = {
        "fe": lambda L: L.call("lh_stft_conv_in", P(mix), P(conv_in), P(conv_out), P(pk["wfb_t"]), P(pk["conv_w"]), P(pk["conv_b"]),
                               P(xa), B, T, ns, st),
        "intra": lambda L: L.call("lh_intra_block", P(xa), P(bp["intra_w16"]), P(bp["intra_b16"]), P(bp["intra_lin_w2"]),
                                  P(bp["intra_lin_b"]), P(xb), B * T, st),
        "inter": lambda L: L.call("lh_inter_block", P(xb), P(bp["inter_w8"]), P(bp["inter_b16"]), P(bp["inter_lin_wu"]),
                                  P(bp["inter_lin_b"]), P(h0), P(c0), P(hN), P(cN), P(xc), B, T, st),
        "qkv": lambda L: L.call("lh_qkv_proj_ln", P(xc), P(bp["qkv_w"]), P(bp["qkv_b"]), P(bp["qkv_slopes"]), P(bp["lnq_w"]),
                                P(bp["lnq_b"]), P(bp["lnk_w"]), P(bp["lnk_b"]), P(bp["lnv_w"]), P(bp["lnv_b"]), P(ws["q"]),
                                P(ws["kx"]), P(ws["vx"]), None, B, T, st),
        "attn": lambda L: L.call("lh_local_attn", P(ws["q"]), P(ws["kx"]), P(ws["vx"]), P(m), B, T, st),
        "proj": lambda L: L.call("lh_proj_ln_res", P(m), P(bp["proj_w"]), P(bp["proj_b"]), P(bp["proj_slope"]), P(bp["proj_ln_w"]),
                                 P(bp["proj_ln_b"]), P(xc), None, P(xo), B, T, st),
        "taps": lambda L: L.call("lh_proj_ln_res_taps", P(m), P(bp["proj_w"]), P(bp["proj_b"]), P(bp["proj_slope"]),
                                 P(bp["proj_ln_w"]), P(bp["proj_ln_b"]), P(xc), P(pk["deconv_w"]), P(ptaps), P(fmax), B, T, st),
        "be": lambda L: L.call("lh_taps_istft", P(ptaps), P(fmax), P(pk["deconv_w"]), P(pk["deconv_b"]), P(pk["wfb_dec"]), P(y),
                               P(flag), 1, B, T, st),
    }
    outs = {"fe": [xa], "intra": [xb], "inter": [xc, hN, cN], "qkv": [ws["q"], ws["kx"], ws["vx"]], "attn": [m], "proj": [xo],
            "taps": [ptaps, fmax], "be": [y]}
    order = list(calls)
    # a forward's order of stages, the closing stage in both its forms (each behind an attention launch, as in a forward)
    chain = ["fe", "intra", "inter", "qkv", "attn", "proj", "attn", "taps", "be"]
    clabel = ["fe", "intra", "inter", "qkv", "attn", "proj", "attn'", "taps", "be"]

    base = _cabi.Lib(build.LIB)
    base.call("lh_set_tuning", 19, 0)
    _cabi.selftest_device(base, 0)
    libs = [("plain", 0, base), ("A/A", 0, base)]
    for mk in masks:
        L = _cabi.Lib(lib_path(mk))
        L.call("lh_set_tuning", 19, 2)
        libs.append((f"{mk:#05x} {names(mk)}", mk, L))

    # real data in every workspace, and the bit-identity of every variant against it
    for s in order:
        calls[s](base)
    torch.cuda.synchronize()
    ref = {s: [t.clone() for t in outs[s]] for s in order}
    for name, mk, L in libs[2:]:
        for s in order:
            if STAGE_BITS[s] & mk:
                for t in outs[s]:
                    t.zero_()
                calls[s](L)
                torch.cuda.synchronize()
                same = all(torch.equal(a, b) for a, b in zip(outs[s], ref[s]))
                print(f"bits  {s:6s} {name:40s} {'identical' if same else 'DIFFERENT'}", flush=True)
                if not same:
                    raise SystemExit(1)
    print(f"B = {B}, T = {T}; {rounds} rounds, {group} calls per stage group; times in us per call (chain: per chain)")

    def timed(fns, L):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for f in fns:
            f(L)
        e1.record()
        return e0, e1

    def report(label, per, n_calls):
        t = {k: np.array([a.elapsed_time(b) for a, b in v]) * 1e3 / n_calls for k, v in per.items()}
        p50 = {k: float(np.percentile(v, 50)) for k, v in t.items()}
        sc = float(np.percentile(t["plain"], 90) - np.percentile(t["plain"], 10)) / 2
        for k in t:
            dlt = p50[k] - p50["plain"]
            verdict = "" if k == "plain" else ("  GAIN" if dlt < -3 * sc else "  LOSS" if dlt > 3 * sc else "  within 3x scatter")
            print(f"{label:9s} {k:52s} p50 {p50[k]:9.2f}   delta {dlt:+8.2f}   baseline scatter {sc:6.2f}{verdict}", flush=True)

    for s in order:
        use = [l for l in libs if l[1] == 0 or STAGE_BITS[s] & l[1]]
        if len(use) == 2:
            continue
        per = {l[0]: [] for l in use}
        for r in range(rounds + 3):
            for k in range(len(use)):                      # rotated: no library always runs behind the same neighbour
                name, mk, L = use[(k + r) % len(use)]
                ev = timed([calls[s]] * group, L)
                if r >= 3:
                    per[name].append(ev)
        torch.cuda.synchronize()
        report(s, per, group)
    # the chain, with an event at every stage boundary (ten records per chain, the same for every library): each stage's time
    # with the cache in the state its predecessor left, and the chain's
    per = {c: {l[0]: [] for l in libs} for c in clabel + ["chain"]}
    for r in range(rounds + 3):
        for k in range(len(libs)):
            name, mk, L = libs[(k + r) % len(libs)]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(chain) + 1)]
            ev[0].record()
            for i, c in enumerate(chain):
                calls[c](L)
                ev[i + 1].record()
            if r >= 3:
                for i, c in enumerate(clabel):
                    per[c][name].append((ev[i], ev[i + 1]))
                per["chain"][name].append((ev[0], ev[-1]))
    torch.cuda.synchronize()
    for c in clabel + ["chain"]:
        report(("in " if c != "chain" else "") + c, per[c], 1)


def cmd_sweep(batches, rounds):
    import numpy as np
    import torch
    from lookoncetohear_amd import _cabi, config, synth
    from lookoncetohear_amd.net import Net

    dev = torch.device("cuda", 0)
    net = Net(**config.TSH_PARAMS).eval()
    net.load_state_dict(config.separator_weights(0), strict=True)
    net = net.to(dev)
    lib = _cabi.load()
    d = synth.batch(list(range(8)), 80000)
    print("B   frame-stream MB   ms off (p50, scatter)   ms on (p50)   delta us   verdict")
    with torch.no_grad():
        for B in batches:
            mix = d["mixture"].repeat((B + 7) // 8, 1, 1)[:B].contiguous().to(dev)
            emb = d["embedding_gt"].repeat((B + 7) // 8, 1, 1)[:B].contiguous().to(dev)
            t = {0: [], 2: []}
            for r in range(rounds + 3):
                for v in ((0, 2) if r % 2 == 0 else (2, 0)):
                    lib.call("lh_set_tuning", 19, v)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    net(mix, emb)
                    e1.record()
                    if r >= 3:
                        t[v].append((e0, e1))
            torch.cuda.synchronize()
            lib.call("lh_set_tuning", 19, 1)
            ms = {v: np.array([a.elapsed_time(b) for a, b in t[v]]) for v in t}
            off, on = float(np.percentile(ms[0], 50)), float(np.percentile(ms[2], 50))
            sc = float(np.percentile(ms[0], 90) - np.percentile(ms[0], 10)) / 2
            dlt = (on - off) * 1e3
            verdict = "on wins" if dlt < -3e3 * sc else "off wins" if dlt > 3e3 * sc else "within 3x scatter"
            print(f"{B:3d} {B * 625 * 97 * 64 * 4 / 2**20:10.0f}   {off:8.3f} {sc:6.3f}   {on:8.3f}   {dlt:+8.0f}   {verdict}"
                  f"   windows {net._n_time_chunks(B, 625, 1)}", flush=True)
            net._ws.clear()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {"--batch": 32, "--rounds": 40, "--group": 4}
    for k in list(opt):
        if k in args:
            opt[k] = int(args[args.index(k) + 1])
            del args[args.index(k):args.index(k) + 2]
    opt["--rounds"] = opt["--rounds"] if "--rounds" in sys.argv else (12 if args[:1] == ["sweep"] else 40)
    if args[:1] == ["sweep"]:
        cmd_sweep([int(a) for a in args[1:]] or [4, 8, 12, 16, 24, 32], opt["--rounds"])
        sys.exit(0)
    masks = [int(a, 16) for a in args[1:]] or [1 << i for i in range(len(STREAMS))]
    if args and args[0] == "build":
        cmd_build(masks)
    elif args and args[0] == "run":
        cmd_run(masks, opt["--batch"], opt["--rounds"], opt["--group"])
    else:
        sys.exit(__doc__)
