#!/usr/bin/env python3
"""ms per launch of the encoder's 512 -> 512 stride-2 3x3 conv at 64^2 -> 32^2, 16 images (the gather kernel's largest launch): the 8-wave
kernel (E4S_GATHER_1W=0), the one-wave-per-SIMD kernel, and -- on a library built with E4S_BUILD_ABLATIONS=1 -- its variants
E4S_GATHER_1W_VAR = 1 no A staging, 2 no weight loads, 3 MFMAs only (WRONG results by construction).  Interleaved rounds in one process;
prints one JSON line (median and min per form).

    E4S_BUILD_ABLATIONS=1 E4S_BUILD_OUT=tools/bin/libe4s_abl.so python -m e4s_amd.build
    E4S_LIB_PATH=tools/bin/libe4s_abl.so python tools/gather1w_ablate.py"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from e4s_amd import kernels as K  # noqa: E402

FORMS = {"8wave": {"E4S_GATHER_1W": "0"}, "1wave": {}, "no_A_staging": {"E4S_GATHER_1W_VAR": "1"}, "no_B_loads": {"E4S_GATHER_1W_VAR": "2"},
         "mfma_only": {"E4S_GATHER_1W_VAR": "3"}}


def main():
    b, h, cin, cout, reps, rounds = 16, 64, 512, 512, 10, 5
    g = torch.Generator().manual_seed(1)
    x = torch.randn(b, h, h, cin, generator=g).cuda()
    w = (torch.randn(1, 9, cout, cin, generator=g) / (cin * 9) ** 0.5).cuda()
    ws, wf = K.split_bf16x2(w), K.gather_frag_bf16x2(w)
    times = {k: [] for k in FORMS}
    for r in range(rounds + 1):
        for name, env in FORMS.items():
            for k in ("E4S_GATHER_1W", "E4S_GATHER_1W_VAR"):
                os.environ.pop(k, None)
            os.environ.update(env)
            K.conv_mfma(x, w, cout, istride=2, ntaps=9, w_split=ws, w_frag=wf)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                K.conv_mfma(x, w, cout, istride=2, ntaps=9, w_split=ws, w_frag=wf)
            t1.record()
            torch.cuda.synchronize()
            if r:                      # round 0 warms up
                times[name].append(t0.elapsed_time(t1) / reps)
    print(json.dumps({"shape": "512->512 3x3 stride 2, 64^2->32^2, 16 images", "ms_per_launch": {
        k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4)} for k, v in times.items()}}))


if __name__ == "__main__":
    main()
