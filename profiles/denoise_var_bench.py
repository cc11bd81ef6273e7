"""rt_denoise_variance against rt_denoise on config 3's scene (pretty_tlas) at 1920x1080 and 3840x2160, five iterations each.
  python3 profiles/denoise_var_bench.py [--rounds N] [--json out.json] [--root <checkout>]          (GPU box, repository root)
The frame: 4 whole path frames with the statistics on (every pixel's count is 4, so rt_denoise(4) filters the same means).  The two calls
are alternated, three rounds; a round times BATCH back-to-back calls of one of them between two stream synchronisations on the host clock
and divides (the calls queue their launches without synchronising, so the figure is the kernels' time on the stream: k_denoise_var_init +
5 x k_denoise_var_atrous against 5 x k_denoise_atrous).  Reported: the median of the three rounds, and the bound of one iteration from
the shapes: tap bytes through L1 (25 taps x 64 B of colour, position, normal and albedo, plus the prefilter's 8 x (16 + 4) B) over the
64 B/clk/CU peak, and the unique HBM bytes.  Per-kernel times: one run of this script under rocprofv3 --kernel-trace --stats.
--root measures another checkout's library (a measurement build: profiles/patches/denoise_var_prefilter_pass.diff)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import importlib  # noqa: E402

HBM_PEAK = 8.0e12        # B/s, MI355X HBM3E
L1_PEAK = 256 * 64 * 2.4e9  # B/s: 256 CUs x 64 B/clk (one 64-B line per CU per clock) x 2.4 GHz
BATCH = 10


def timed(r, call):
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(BATCH):
        call()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3 / BATCH


def run(ha, scenes, w, h, rounds):
    r = ha.HostRenderer(w, h)
    scenes.pretty_tlas(r.scene, 8)
    r.commit()
    r.stats_enable(True)
    r.clear()
    r.render(ha.RT_MODE_PATH, 0, 4)
    r.render_aovs(0.001)
    calls = dict(denoise_variance=lambda: r.denoise_variance(None), denoise=lambda: r.denoise(4, None))
    for c in calls.values():
        for _ in range(3):
            c()
    ms = dict((k, []) for k in calls)
    for _ in range(rounds):
        for k, c in calls.items():
            ms[k].append(timed(r, c))
    n = w * h
    it = ha.DENOISE_VAR_DEFAULTS["iterations"]
    med = dict((k, float(np.median(v))) for k, v in ms.items())
    taps = n * (25 * 64 + 8 * 20)
    hbm = n * 5 * 16
    per_it = med["denoise_variance"] / it  # (the init pass, 28 B read + 16 B written per pixel, is inside: it is not priced apart here)
    out = dict(width=w, height=h, pixels=n, rounds=rounds, batch=BATCH, iterations=it,
               denoise_variance_ms=dict(median=round(med["denoise_variance"], 4), all=[round(v, 4) for v in ms["denoise_variance"]]),
               denoise_ms=dict(median=round(med["denoise"], 4), all=[round(v, 4) for v in ms["denoise"]]),
               ratio=round(med["denoise_variance"] / med["denoise"], 3),
               per_iteration=dict(ms=round(per_it, 4), unique_hbm_bytes=hbm, tap_bytes_l1=taps,
                                  hbm_frac_of_peak=round(hbm / (per_it * 1e-3) / HBM_PEAK, 4),
                                  l1_frac_of_peak=round(taps / (per_it * 1e-3) / L1_PEAK, 4)),
               peaks=dict(hbm_Bps=HBM_PEAK, l1_Bps=L1_PEAK), build=r.build_info())
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--root", default=HERE, help="the checkout whose library is measured")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    ha.build()
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    res = [run(ha, scenes, w, h, a.rounds) for w, h in ((1920, 1080), (3840, 2160))]
    for r in res:
        print(json.dumps(r))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
