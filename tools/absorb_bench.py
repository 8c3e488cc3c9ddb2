"""tools/absorb_bench.py [--out profiles/absorb.md] — records of any length hashed on the MI355X (include/gstark_absorb.h), written as a
profile: permutations/s of `absorbMany` next to `hashMany` of the same parameter set in the same process.

  sets      lib128's Poseidon (width 6, 128-bit field, rate 4), rescue4x128 (width 4, 128-bit field, rate 2), lib224's Poseidon (width 3,
            224-bit field, rate 2)
  rows      2^20 records of L = rate, 4 * rate and 16 * rate elements: 1, 4 and 16 permutations per record
  layouts   rows (a 2^20 x L matrix) and columns (the register-major L x 2^20 matrix)
  hashMany  2^20 rows of `rate` inputs, the same digest size: one permutation per row; the ratio is (absorb permutations/s) / (hashMany
            permutations/s), expected within 10 % of 1 (a block adds `rate` additions and `rate` loads to thousands of products)

Times are host clock around `reps` back-to-back launches that end in one gs_sync, after a warm-up of the same shape; every window is at
least --window seconds long.  Register counts, scratch and waves per SIMD are the compiler's -Rpass-analysis=kernel-resource-usage
remarks for gfx950 (RESOURCES below; refresh them when a kernel changes).  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from genstark_amd import _abi, lib128, lib224          # noqa: E402
from genstark_amd._abi import Backend                  # noqa: E402
from genstark_amd.field import Matrix, PrimeField      # noqa: E402
from genstark_amd.rescue_hash import rescue4x128       # noqa: E402
from sponge_bench import timed                         # noqa: E402

ROWS = 1 << 20
# (absorb kernel, its one-permutation counterpart): VGPRs, AGPRs, SGPRs, scratch bytes per lane, waves per SIMD, LDS bytes per workgroup
RESOURCES = {
    'lib128 Poseidon': (('k_hades_absorb<6>', 113, 0, 106, 0, 4, 0), ('k_hades_hash<6>', 112, 0, 106, 0, 4, 20480)),
    'rescue4x128': (('k_rescue_absorb<4>', 105, 0, 88, 0, 4, 0), ('k_rescue_spread<4>', 97, 0, 62, 0, 4, 0)),
    'lib224 Poseidon': (('k_hades_absorb<3>', 145, 0, 106, 0, 3, 0), ('k_hades_hash<3>', 141, 0, 106, 0, 3, 16384)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'absorb.md'))
    ap.add_argument('--window', type=float, default=0.25)
    args = ap.parse_args()
    lines = ['# Records of any length: absorbMany against hashMany (tools/absorb_bench.py)', '',
             f'2^20 records per launch.  Time per launch: host clock around back-to-back launches ending in one synchronise, after a warm-up.',
             'Ratio: permutations/s of `absorbMany` over permutations/s of `hashMany` (2^20 rows of `rate` inputs, same digest) in the same process.', '']
    for name, modulus, make, family, digest in (('lib128 Poseidon', None, lib128.poseidon, 'hades', 2), ('rescue4x128', None, rescue4x128, 'rescue', 1),
                                                ('lib224 Poseidon', _abi.MODULUS_224, lib224.poseidon, 'hades', 1)):
        be = Backend(device=0, modulus=modulus)
        f = PrimeField(backend=be)
        h = make(f)
        rate = h.width - 1 if h.width <= 3 else h.width - 2
        options = (1,) if family == 'rescue' else ()
        series = f.getPowerSeries(3, ROWS * 16 * rate)                  # inputs made on the device: distinct non-trivial elements
        out = Matrix(be, ROWS, digest)
        src = Matrix(be, ROWS, rate, owner=series._owner)
        hash_options = (1, 0) if family == 'rescue' else ()
        t_hash, reps = timed(be, lambda: be.call(f'gs_{family}_hash', h.handle(), C.c_void_p(src.ptr), ROWS, rate, digest, *hash_options, C.c_void_p(out.ptr)), args.window)
        base = ROWS / t_hash
        lines += [f'## {name}: width {h.width}, rate {rate}, digest {digest}', '',
                  '| kernel | VGPRs | AGPRs | SGPRs | scratch bytes/lane | waves per SIMD | LDS bytes/workgroup |', '|---|---|---|---|---|---|---|']
        lines += ['| `' + r[0] + '` | ' + ' | '.join(str(v) for v in r[1:]) + ' |' for r in RESOURCES[name]]
        lines += ['', f'`hashMany`, 2^20 rows of {rate}: {t_hash * 1e3:.3f} ms per launch ({reps} reps), {base / 1e6:.2f} M permutations/s.', '',
                  '| L | permutations per record | layout | reps | ms per launch | M permutations/s | ratio to hashMany |', '|---|---|---|---|---|---|---|']
        for blocks in (1, 4, 16):
            length = blocks * rate
            for layout, strides in (('rows', (length, 1)), ('columns', (1, ROWS))):
                t, reps = timed(be, lambda: be.call(f'gs_{family}_absorb', h.handle(), C.c_void_p(series.ptr), ROWS, length, *strides, rate, digest, *options,
                                                    C.c_void_p(out.ptr)), args.window)
                rate_s = ROWS * blocks / t
                lines.append(f'| {length} | {blocks} | {layout} | {reps} | {t * 1e3:.3f} | {rate_s / 1e6:.2f} | {rate_s / base:.3f} |')
        lines.append('')
        del series, src, out
        be.close()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
