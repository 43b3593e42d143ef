"""The decode step's kernels get their leading arguments preloaded into user SGPRs ("leading arguments preloaded").

hipcc preloads only leading PLAIN parameters (pointers, integers), never a by-value struct, and says how many dwords it granted in
`.amdhsa_user_sgpr_kernarg_preload_length`.  This compiles the four translation units of the step to device assembly with the
project's own FLAGS and pins that figure per converted kernel: an edit that turns a struct back into the first parameter (length 0),
drops the build flag, or pushes what the first loads need behind the granted dwords fails here, without a GPU.

Expected dword counts, read from the assembly (16 user SGPRs, 2 of them the argument segment's address: 14 dwords at most):
  gemm_dec32x_k          13  Wp 2, w_plane 2, N 1, w_nt 1, n_active 2, Ap 2, a_plane 2, M 1
  attention_k            14  dbg 2, n_active 2, desc 2, q_per_b 1, desc_covers_all 1, kc 2, vc 2, cmax 1, grid_x 1   (qkv, out: fetched)
  embed_codes_k          14  zero_p 2, row_map_out 2, finish 2, order 2, n_active 2, row_map 2, len 2
  sample_k               14  dbg 2, desc 2, n_active 2, row_map 2, len 2, tcap 1, T 1, prompt_len 2
  gemm_dec32_*_k         12  Wp 2, Ap 2, N 1, w_nt 1, norm_w 2, n_active 2, M 1, K 1
  gemm_dec_k             14  dbg 2, Wp 2, Ap 2, N 1, K 1, w_nt 1, a_early 1, n_active 2, M 1, grid_x 1
"""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from chattts_amd import build as B

# mangled-name prefix of the kernel (every template instantiation of it) -> dwords the compiler must grant
EXPECT = {
    "decode32x.hip": {"_Z13gemm_dec32x_kI": 13},
    "decode.hip": {"_Z10gemm_dec_kI": 14},
    "decode32.hip": {"_Z12gemm_dec32_kI": 12, "_Z16gemm_dec32_m16_kI": 12, "_Z18gemm_dec32_rms16_kI": 12, "_Z20gemm_dec32_fnorm16_k": 12},
    "gpt.hip": {"_Z11attention_kI": 14, "_Z13embed_codes_k": 14, "_Z8sample_k": 14},
}
# the headline step's own instantiation must be among the attention kernels: f32 KV cache, 4 waves, packed split (x3) output
HEADLINE_ATTENTION = "_Z11attention_kIfLi4E5x3p_tLb1E"


def _assembly(src, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, *B.FLAGS, "--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", out], check=True, capture_output=True, timeout=900)
    with open(out) as fh:
        text = fh.read()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        n = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", m.group(2))
        found[m.group(1)] = int(n.group(1)) if n else 0
    return found


@pytest.fixture(scope="module")
def preload(tmp_path_factory):
    d = tmp_path_factory.mktemp("preload_asm")
    with ThreadPoolExecutor(max_workers=4) as pool:
        res = list(pool.map(lambda s: _assembly(s, str(d / s.replace(".hip", ".s"))), EXPECT))
    return dict(zip(EXPECT, res))


def test_build_flags_ask_for_preload():
    assert "-amdgpu-kernarg-preload-count=16" in B.FLAGS and B.FLAGS[B.FLAGS.index("-amdgpu-kernarg-preload-count=16") - 1] == "-mllvm"


@pytest.mark.parametrize("src", list(EXPECT))
def test_step_kernels_preload_what_their_first_loads_need(preload, src):
    kernels = preload[src]
    for prefix, want in EXPECT[src].items():
        inst = {k: v for k, v in kernels.items() if k.startswith(prefix)}
        assert inst, (src, prefix, "no such kernel in the assembly")
        for name, got in inst.items():
            assert got > 0, (name, "no leading argument is preloaded: a by-value struct is the first parameter again?")
            assert got == want, (name, got, want)
    if src == "gpt.hip":
        assert any(k.startswith(HEADLINE_ATTENTION) for k in kernels), "the f32x3 step's attention kernel is gone"
