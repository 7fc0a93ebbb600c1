#!/usr/bin/env python3
"""How far the two paths of the bilateral upsample that take their exponentials
on the device (bilateral_kernel: the stand-alone smvs_bilateral_upsample, and
smvs_ctx_sgm_init_depth with kernel_size > 7) are from the CPU oracle, over the
cases of tests/bilateral_cases.py (the contrast pair excepted, as in
tests/test_gpu_bilateral.py).  Prints the report of
profiles/bilateral_forms_parity.txt; an argument names a file to write it to."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import smvs_amd
from oracle import pyoracle
import bilateral_cases as bc

lines = ["bilateral_kernel (exponentials on the device: exp in double, rounded once) against",
         "oracle.bilateral_upsample (glibc expf), tests/bilateral_cases.py without the contrast pair.",
         "Per case: pixels with depth, of them bit-identical, largest difference in ulps of the",
         "oracle's value and in units of max|want| (the tests' bound: 1e-5).", ""]
worst = {}


def row(path, case, got, want):
    assert np.array_equal(got == 0, want == 0), (path, case.name)
    filled = want != 0
    n = int(filled.sum())
    u = bc.ulps(got, want)
    same = int((u[filled] == 0).sum())
    scale = float(np.abs(want).max())
    rel = float(np.abs(got - want).max()) / scale if scale > 0 else 0.0
    w = worst.setdefault(path, dict(ulps=0, rel=0.0, n=0, same=0))
    w["ulps"] = max(w["ulps"], int(u.max()))
    w["rel"] = max(w["rel"], rel)
    w["n"] += n
    w["same"] += same
    lines.append("%-12s %-40s %8d %8d  %2d ulp  %.2e" % (path, case.name, n, same, int(u.max()), rel))


for case in bc.CASES + bc.SECOND_TRIP:
    if case.kind == "contrast":
        continue
    img, dm = bc.inputs(case)
    ci = bc.to_float(img)
    want = pyoracle.bilateral_upsample(dm, ci, case.sigma, case.kernel_size)
    row("stand-alone", case, smvs_amd.bilateral_upsample(dm, ci, case.sigma, case.kernel_size), want)
    if case.kernel_size > 7:
        ctx = smvs_amd.ViewContext(case.w, case.h, 1)
        ctx.upload_image(-1, img)
        row("context", case, ctx.sgm_init_depth(dm, case.sigma, case.kernel_size), want)
        ctx.close()
lines.append("")
for path, w in worst.items():
    lines.append("%-12s worst: %d ulp, %.2e max|want|; %d of %d pixels with depth bit-identical (%.2f %%)"
                 % (path, w["ulps"], w["rel"], w["same"], w["n"], 100.0 * w["same"] / max(w["n"], 1)))
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text)
