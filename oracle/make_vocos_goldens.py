"""BUILD-CONTAINER ONLY.  tests/golden/vocos_ref.npz: the Vocos decode with the backbone's blocks evaluated by the
REAL reference class -- `ConvNeXtBlock` of the reference's ChatTTS/model/dvae.py:14-66, "copied from Vocos", imported through
oracle/ref_harness.py and never copied -- instead of our restatement of it.  Everything around the blocks is torch's own modules composed
as vocos.models.VocosBackbone / vocos.heads.ISTFTHead compose them (the `vocos` package is not installed): Conv1d(100, 512, 7, padding=3),
LayerNorm(512, eps=1e-6), 8 blocks (512, 1536, kernel 7, dilation 1), LayerNorm, Linear(512, 1026), then exp, clip(max=1e2), torch.polar,
torch.istft(1024, 256, 1024, window, center=True).  What stays restated is therefore the module order, the state dict's key names
(`backbone.convnext.i.gamma` is the block's `.weight`) and the head.

The fixture holds, for F = 2, 9, 66 frames, the mel [2, 100, F] (torch.randn, generator seed F) and the waveform [2, 256 (F - 1)]: data only.

    python -m oracle.make_vocos_goldens
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from chattts_amd import weights as W
from oracle import ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "vocos_ref.npz")
FRAMES = (2, 9, 66)
N_BLOCKS = 8


def mel_input(F: int) -> torch.Tensor:
    """[2, 100, F], N(0, 1), generator seed F"""
    return torch.randn((2, 100, F), generator=torch.Generator().manual_seed(F), dtype=torch.float32)


class Vocos(nn.Module):
    def __init__(self, sd: dict):
        super().__init__()
        block = ref_harness.ref_modules()["dvae"].ConvNeXtBlock
        self.embed = nn.Conv1d(100, 512, 7, padding=3)
        self.norm = nn.LayerNorm(512, eps=1e-6)
        self.convnext = nn.ModuleList([block(512, 1536, 7, 1) for _ in range(N_BLOCKS)])
        self.final_layer_norm = nn.LayerNorm(512, eps=1e-6)
        self.out = nn.Linear(512, 1026)
        self.register_buffer("window", sd["head.istft.window"].clone())
        own = {}
        for k, v in sd.items():
            if k.startswith("backbone."):
                k = k[len("backbone."):]
                own[k[:-len("gamma")] + "weight" if k.endswith(".gamma") else k] = v
            elif k.startswith("head.out."):
                own[k[len("head."):]] = v
        own["window"] = sd["head.istft.window"]
        self.load_state_dict(own)          # strict: every key of the synthetic state dict has exactly one home

    def forward(self, mel: torch.Tensor) -> torch.Tensor:
        x = self.embed(mel)
        x = self.norm(x.transpose(1, 2)).transpose(1, 2)
        for blk in self.convnext:
            x = blk(x)
        x = self.final_layer_norm(x.transpose(1, 2))
        mag, p = self.out(x).transpose(1, 2).chunk(2, dim=1)
        mag = torch.clip(torch.exp(mag), max=1e2)
        return torch.istft(torch.polar(mag, p), 1024, 256, 1024, self.window, center=True)


@torch.inference_mode()
def build() -> dict:
    """the fixture's arrays, from the reference's class: {"F<n>.mel": [2, 100, n], "F<n>.wav": [2, 256 (n - 1)]}.  On ONE thread: torch's
    CPU GEMMs and FFT split their sums by the thread count (the last bit moves, 1e-7 on this waveform), and the rebuild in
    tests/test_vocos_reference_golden.py asks for the same bits on a machine with another number of cores."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        model = Vocos(W.synthetic_vocos()).eval()
        out = {}
        for F in FRAMES:
            mel = mel_input(F)
            out[f"F{F}.mel"] = mel.numpy().copy()
            out[f"F{F}.wav"] = model(mel).numpy().copy()
        return out
    finally:
        torch.set_num_threads(threads)


def main():
    from oracle import codec_np, torch_port
    out = build()
    sd = W.synthetic_vocos()
    nsd = {k: v.numpy() for k, v in sd.items()}
    for F in FRAMES:
        mel, wav = out[f"F{F}.mel"], out[f"F{F}.wav"]
        rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - wav) ** 2)))
        print(f"F={F}: wav rms {float(np.sqrt(np.mean(wav.astype(np.float64) ** 2))):.2e}  torch_port-vs-reference "
              f"{rms(torch_port.vocos_decode(sd, torch.from_numpy(mel)).numpy()):.2e}  codec_np-vs-reference "
              f"{rms(codec_np.vocos_decode(nsd, np.ascontiguousarray(mel.transpose(0, 2, 1)))):.2e}")
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
