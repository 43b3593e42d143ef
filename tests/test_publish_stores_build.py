"""The decode step's kernels publish their results with write-through stores ("results published write-through").

common.hpp's publishN helpers store with the `sc1` bit, so that the release at the end of a launch finds the L2 clean;
-DCTTS_PLAIN_PUBLISH=1 turns them back into plain stores (the A/B build).  This compiles the translation units of the headline
(`f32x3`) step to device assembly with the project's own FLAGS, once per setting, and pins per kernel:
  * default build: every global store of the kernel carries sc1, except the listed ones that are no results of the step -- the 8-byte
    time stamps of the phase probes (`dbg`), the arrival words the step's first kernel zeroes;
  * the kernels that were measured slower with write-through stores and therefore stay plain (the sampler, the heads GEMM: `profiles/r9C`)
    carry none;
  * with CTTS_PLAIN_PUBLISH=1 no store of any of them carries sc1;
  * in both builds the kernels use no scratch and keep the preloaded argument dwords of tests/test_kernarg_preload_build.py.
An edit that adds a plain store to an epilogue, drops the helper, or makes a kernel spill fails here, without a GPU."""
import os
import re
import subprocess
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import pytest

from chattts_amd import build as B

# source -> mangled-name prefix -> (publishes, {instruction: count}, preloaded dwords); the counts: for a publishing kernel the plain stores it
# may keep, for a kernel that stays plain the write-through stores it may have
STEP = {
    "decode32x.hip": {"_Z13gemm_dec32x_kI": (True, {}, 13)},
    "decode32.hip": {"_Z20gemm_dec32_fnorm16_k": (False, {}, 12)},
    "gpt.hip": {
        "_Z13embed_codes_k": (True, {"global_store_dword": 1}, 14),            # step_zero's arrival words
        "_Z11attention_kIfLi4E5x3p_tLb1E": (True, {"global_store_dwordx2": 7}, 14),   # ASTAMP time stamps
        # (the row of the embedding fold, CTTS_EMBED_FOLD=1, off: emit_row + the RoPE factors, shared with embed_codes_k)
        "_Z8sample_k": (False, {"global_store_dwordx4": 2, "global_store_dwordx2": 3, "global_store_dword": 2}, 14),
    },
}
# what the publishing kernels must at least store write-through (the widths their results have)
MUST = {
    "_Z13gemm_dec32x_kI": set(),                                                  # per epilogue: _must() below
    "_Z13embed_codes_k": {"global_store_dwordx4", "global_store_dwordx2", "global_store_dword"},   # x32 / desc, the planes, ssq / rope / n_active
    "_Z11attention_kIfLi4E5x3p_tLb1E": {"global_store_short"},
}


def _must(prefix, name):
    if prefix != "_Z13gemm_dec32x_kI":
        return MUST[prefix]
    epi = re.match(r"_Z13gemm_dec32x_kILi\d+ELi\d+ELb[01]ELi(\d+)E", name).group(1)
    # 100: q and the K / V append (f32); 2: the SiLU * up planes; 1: residual + sum of squares (f32) and the planes
    return {"100": {"global_store_dword"}, "2": {"global_store_short"}, "1": {"global_store_dword", "global_store_short"}}[epi]


def _kernels(src, out, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, *B.FLAGS, *extra, "--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", out], check=True, capture_output=True, timeout=900)
    with open(out) as fh:
        text = fh.read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        stores = [ln.strip() for ln in m.group(2).splitlines() if re.match(r"\s*(global|buffer|flat)_store_", ln)]
        found[m.group(1)] = {"wt": Counter(s.split()[0] for s in stores if re.search(r"\bsc1\b", s)),
                             "plain": Counter(s.split()[0] for s in stores if not re.search(r"\bsc1\b", s)),
                             "nt": sum(1 for s in stores if re.search(r"\bnt\b", s)),
                             "scratch_ops": len(re.findall(r"^\s*scratch_(load|store)_", m.group(2), re.M))}
    for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        if m.group(1) in found:
            n = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", m.group(2))
            p = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2))
            found[m.group(1)]["preload"] = int(n.group(1)) if n else 0
            found[m.group(1)]["scratch_bytes"] = int(p.group(1)) if p else -1
    return found


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("publish_asm")
    jobs = [(src, tag, extra) for src in STEP for tag, extra in (("wt", []), ("plain", ["-DCTTS_PLAIN_PUBLISH=1"]))]
    with ThreadPoolExecutor(max_workers=6) as pool:
        res = list(pool.map(lambda j: _kernels(j[0], str(d / (j[1] + "_" + j[0].replace(".hip", ".s"))), j[2]), jobs))
    return {(j[0], j[1]): r for j, r in zip(jobs, res)}


def _instances(asm, src, tag, prefix):
    inst = {k: v for k, v in asm[(src, tag)].items() if k.startswith(prefix)}
    assert inst, (src, prefix, "no such kernel in the assembly")
    return inst


@pytest.mark.parametrize("src", list(STEP))
def test_results_leave_write_through(asm, src):
    for prefix, (publishes, plain_ok, _) in STEP[src].items():
        for name, k in _instances(asm, src, "wt", prefix).items():
            assert k["nt"] == 0, (name, "a non-temporal store in a step kernel: never combined with handed-off data")
            if not publishes:
                assert k["wt"] == Counter(plain_ok), (name, "measured slower with write-through stores: stays on plain stores", dict(k["wt"]))
                continue
            assert sum(k["wt"].values()) > 0 and _must(prefix, name) <= set(k["wt"]), (name, dict(k["wt"]))
            assert k["plain"] == Counter(plain_ok), (name, "a result of the step leaves through a plain store", dict(k["plain"]))


@pytest.mark.parametrize("src", list(STEP))
def test_plain_switch_removes_every_write_through_store(asm, src):
    for prefix in STEP[src]:
        for name, k in _instances(asm, src, "plain", prefix).items():
            assert not k["wt"], (name, dict(k["wt"]))
            assert sum(k["plain"].values()) > 0, name


@pytest.mark.parametrize("tag", ["wt", "plain"])
@pytest.mark.parametrize("src", list(STEP))
def test_no_scratch_and_the_same_preloaded_arguments(asm, src, tag):
    for prefix, (_, _, dwords) in STEP[src].items():
        for name, k in _instances(asm, src, tag, prefix).items():
            assert k["scratch_bytes"] == 0 and k["scratch_ops"] == 0, (name, k["scratch_bytes"], k["scratch_ops"])
            assert k["preload"] == dwords, (name, k["preload"], dwords)
