"""The timing loop and the product-cost reader of tools/hades_bench.py and tools/rescue_bench.py.  Not a tool of its own."""
import glob
import json
import os
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMDS, LANES = 1024, 64


def timed(be, launch, window):
    launch()
    be.sync()
    t0 = time.perf_counter()
    launch()
    be.sync()
    once = max(time.perf_counter() - t0, 1e-6)
    reps = max(3, int(window / once) + 1)
    t0 = time.perf_counter()
    for _ in range(reps):
        launch()
    be.sync()
    return (time.perf_counter() - t0) / reps, reps


def product_cost(detail_path):
    """ns per wave-wide 128-bit product at 1 .. 4 waves per SIMD, and where it came from"""
    paths = [detail_path] if os.path.exists(detail_path) else sorted(glob.glob(os.path.join(ROOT, 'profiles', '*bench_detail.json')))[-1:]
    for path in paths:
        table = json.load(open(path)).get('roofline', {}).get('second_roof', {}).get('measured_ns_per_wave_at_1_2_3_4_waves_per_simd', {})
        if 'canonical_limb_fe_mul_for_reference' in table:
            return table['canonical_limb_fe_mul_for_reference'], os.path.relpath(path, ROOT)
    return None, None

