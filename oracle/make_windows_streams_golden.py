"""Records tests/golden/decode_windows_streams_sha256.json: the SHA-256 of every array the cases of
tests/test_gpu_decode_windows_streams_pin.py return.  Needs the MI355X.  Run it twice, in separate processes, from the commit whose
behaviour is to be pinned -- `python -m oracle.make_windows_streams_golden A.json`, then `... B.json --against A.json`: the second run
keeps only the cases on which both agree and names the others."""
import json
import sys

import torch

from chattts_amd import engine as E, weights as W
from tests.test_gpu_decode_windows_pin import digest
from tests.test_gpu_decode_windows_streams_pin import decode_windows_streams_cases


def main(path: str, against=None) -> None:
    sds = W.synthetic_all()
    codec = E.CodecEngine(sds["decoder"], sds["vocos"], torch.device("cuda:0"), gemm="f32")
    cases = {k: digest(v) for k, v in decode_windows_streams_cases(codec).items()}
    differ = []
    if against is not None:
        with open(against) as fh:
            first = json.load(fh)["cases"]
        differ = sorted(k for k in cases if first.get(k) != cases[k])
        cases = {k: v for k, v in cases.items() if k not in differ}
    with open(path, "w") as fh:
        json.dump({"gemm": "f32", "left_out": differ, "cases": cases}, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{len(cases)} cases, {sum(len(v) for v in cases.values())} arrays -> {path}; the two recordings differ on: {differ or 'none'}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[3] if len(sys.argv) > 3 and sys.argv[2] == "--against" else None)
