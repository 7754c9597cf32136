#!/usr/bin/env python3
"""Writes tests/golden/marker_chain_hongo_huber_outliers.json: the marker-chain model on hongo (Main_Calibration's committed
correspondences) with about 5 % of its corners displaced by 30 px (fixed seed), solved with ceres::HuberLoss(2 px) by the numpy
reference tests/marker_loss_ref.py.  The file holds the inputs (so that it is self-contained), every iteration row, the summary
and the final parameters of all C + T + M blocks.

usage: python tools/marker_chain_loss_fixture.py [--check]   (--check: regenerate in memory and compare with the committed file)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import marker_loss_ref as ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "marker_chain_hongo_huber_outliers.json")
FRACTION, PIXELS, SEED, LOSS, SCALE = 0.05, 30.0, 20261015, "huber", 2.0


def build():
    prob = ref.displace_corners(ref.hongo(), FRACTION, PIXELS, SEED)
    mc = ref.MarkerChain(prob, variant=0, loss=LOSS, a=SCALE)
    x, summary, rows = ref.minimise(mc)
    fx = dict(name="hongo_huber_outliers", model="main", outlier_fraction=FRACTION, outlier_pixels=PIXELS, seed=SEED, loss=LOSS, loss_scale=SCALE,
              T=prob["T"], C=prob["C"], M=prob["M"], N=prob["N"], t=prob["t"].tolist(), c=prob["c"].tolist(), m=prob["m"].tolist(),
              obs=prob["obs"].ravel().tolist(), params=prob["params"].tolist(), intr=prob["intr"].ravel().tolist(), marker_side=prob["marker_side"],
              expected=dict(summary=summary, iterations=rows, final_params=mc.full(x).ravel().tolist()))
    return json.dumps(fx, indent=1) + "\n"


def main():
    text = build()
    if "--check" in sys.argv[1:]:
        same = open(OUT).read() == text
        print("identical" if same else "DIFFERS")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", OUT)
    return 0


if __name__ == "__main__":
    sys.exit(main())
