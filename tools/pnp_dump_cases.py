"""Writes the PnPsolver cases (tests/pnp_cases.py) as one binary file for tools/pnp_check_main.cpp, the stand-alone
program that runs the referee and the host build of pnp_math.h over them (under a host sanitizer, for instance).
  python tools/pnp_dump_cases.py cases.bin"""
import pathlib
import struct
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT / "sp-slam_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

import pnp_cases as C  # noqa: E402


def main():
    points, bad, cases = C.build()
    with open(sys.argv[1], "wb") as f:
        f.write(struct.pack("<iiidf", len(points), len(cases), C.RAND_MAX, C.PROBABILITY, C.TH2))
        f.write(C.camera().tobytes() + C.sigma2().tobytes())
        f.write(np.ascontiguousarray(points["xw"], np.float32).tobytes() + bad.tobytes())
        for c in cases:
            mn, mx, eps = c["params"]
            f.write(struct.pack("<iiiiifi", len(c["kun"]), len(c["kf_rows"]), c["rand_iterations"], mn, mx, eps,
                                len(c["calls"])))
            f.write(np.array(c["calls"], np.int32).tobytes())
            for a in (np.ascontiguousarray(c["kun"]), c["match"], c["kf_rows"], c["rand"]):
                f.write(a.tobytes())
    print(f"{len(cases)} cases, {len(points)} rows -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
