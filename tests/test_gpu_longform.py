"""GPU: one 60 s utterance (7 500 frames) offline and as 7 500 8 ms chunks through `Streamer`, against the float64 oracle.
Nothing else in the suite runs past 5 s: this holds the carried recurrences and the 50-slot streaming ring, which wraps 150
times here, against float64 over the whole length, and prints the error per 5 s segment so any growth shows."""
import pytest
import torch

from lookoncetohear_amd import synth
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, SECONDS, SEG = 16000, 60, 5


def test_sixty_seconds_offline_and_streamed_against_fp64(oracle_cfg_sd):
    cfg, sd = oracle_cfg_sd
    net = Net(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    n = SR * SECONDS
    d = synth.batch([11], n)
    mix, emb, tgt = d["mixture"], d["embedding_gt"], d["target"]
    with torch.no_grad():
        y_off = net(mix.to(DEV), emb.to(DEV)).cpu()
        st = net.make_streamer(1, DEV)
        st.set_embedding(emb[:, 0].to(DEV))
        xp = torch.nn.functional.pad(mix, (0, 64)).to(DEV)          # the 64-sample look-ahead of the last chunk
        outs = [st.step(xp[:, :, i * 128:i * 128 + 192]).clone() for i in range(n // 128)]
        torch.cuda.synchronize()
        y_str = torch.cat(outs, -1).cpu()
    ref = O.forward(cfg, sd, mix, emb, dtype=torch.float64, fast_lstm=True)
    assert y_off.shape == y_str.shape == ref.shape
    seg = SR * SEG
    worst = {}
    for name, y in (("offline", y_off), ("streamed", y_str)):
        errs = [(y[..., k:k + seg].double() - ref[..., k:k + seg]).abs().max().item() for k in range(0, n, seg)]
        print(f"{name:>9} max|hip - fp64| per {SEG} s: " + " ".join(f"{e:.2e}" for e in errs))
        dsi = (O.si_snr_i(y.double(), mix.double(), tgt.double()) - O.si_snr_i(ref, mix.double(), tgt.double())).abs().item()
        print(f"{name:>9} |SI-SNRi(hip) - SI-SNRi(fp64)| = {dsi:.2e} dB")
        worst[name] = (max(errs), dsi)
    for name, (e, dsi) in worst.items():
        assert e <= 1e-4, (name, e)
        assert dsi < 0.05, (name, dsi)
