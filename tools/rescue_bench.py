"""tools/rescue_bench.py [--out profiles/rescue.md] [--detail bench_detail.json] — Rescue permutations and trees on the MI355X
(include/gstark_rescue.h), written as a profile.

  permutations/s   the 4 x 128 parameter set of examples/rescue (x^3, 32 rounds) in the modified sponge the tree uses (31 double rounds),
                   form 1 (a thread per permutation) and form 2 (a lane per state element) at 1, 64, 2^10, 2^14 and 2^20 per launch
  chains           the same launches through a library whose inverse S-box chain runs on canonical elements (fe_mul) instead of the
                   lazy five-limb form: `--build-canonical` makes it (csrc/rescue.hip with -DGS_RESCUE_CANONICAL_CHAIN, linked with the
                   other objects of csrc/build; needs only the compiler), the measuring run loads it when it is there
  trees            2^8, 2^16 and 2^20 leaves on the device (leaves in place); 2^8 leaves through the host-integer fallback of
                   RescueMerkleTree on the same machine, and the 2^16-leaf fallback as 2^16 - 1 times its time per hash (a plain loop;
                   `--host-full` runs it whole: about a quarter of an hour)
  product roof     products per permutation (the library's own tally: gs_traffic) x the per-product issue cost of the `second_roof`
                   table of bench_detail.json (bench.py writes it: ns per wave-wide product at 1 .. 4 waves per SIMD, registers only),
                   spread over the chip's 1 024 SIMDs; the fraction is roof time / measured time.  The table prices a general canonical
                   product; most of a chain is squarings, which cost less, so a fraction above 1 is possible: a yardstick, not a bound.
                   Without a table in --detail (bench.py writes it with --full) the latest profiles/*bench_detail.json is used

Times are host clock around `reps` back-to-back launches that end in one gs_sync, after a warm-up of the same shape; every window is at
least --window seconds long.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from genstark_amd._abi import Backend, MODULUS_128                        # noqa: E402
from genstark_amd.field import Matrix, PrimeField, Vector                 # noqa: E402
from genstark_amd.hostfield import HostField                              # noqa: E402
from genstark_amd.rescue_hash import RescueMerkleTree, rescue4x128        # noqa: E402
from sponge_bench import LANES, SIMDS, product_cost, timed     # noqa: E402

CSRC = os.path.join(ROOT, 'genstark_amd', 'csrc')
CANONICAL_LIB = os.path.join(CSRC, 'libgstark_hip_rescue_canonical.so')
COUNTS = (1, 64, 1 << 10, 1 << 14, 1 << 20)
# waves per SIMD of k_rescue_hash<4> / k_rescue_spread<4> in the 128-bit flavour, from -Rpass-analysis=kernel-resource-usage
OCCUPANCY = {1: 5, 2: 4}


def build_canonical():
    units = open(os.path.join(CSRC, 'build.sh')).read().split('UNITS="')[1].split('"')[0].split()
    flags = open(os.path.join(CSRC, 'build.sh')).read().split('FLAGS="')[1].split('"')[0].split()
    obj = os.path.join(CSRC, 'build', 'rescue_canonical.o')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc] + flags + ['-DGS_RESCUE_CANONICAL_CHAIN', '-c', os.path.join(CSRC, 'rescue.hip'), '-o', obj])
    others = [os.path.join(CSRC, 'build', u + '.o') for u in units if u != 'rescue']
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', CANONICAL_LIB, obj] + others + ['-lhiprtc', '-ldl'])
    print('built', CANONICAL_LIB)


def products_per_permutation(be, h, src, out):
    be.traffic(True)
    be.call('gs_rescue_hash', h.handle(), C.c_void_p(src.ptr), 1, 2, 1, 1, 1, C.c_void_p(out.ptr))
    tally = be.traffic()
    be.traffic(False)
    return tally['k_rescue_hash<4>']['units']


def permutation_table(be, h, src, out, window, counts, forms, roof):
    rows = {}
    for count in counts:
        for form in forms:
            t, reps = timed(be, lambda: be.call('gs_rescue_hash', h.handle(), C.c_void_p(src.ptr), count, 2, 1, 1, form, C.c_void_p(out.ptr)), window)
            rows[(count, form)] = (t, reps, roof(count, form))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rescue.md'))
    ap.add_argument('--detail', default=os.path.join(ROOT, 'bench_detail.json'))
    ap.add_argument('--window', type=float, default=0.25)
    ap.add_argument('--build-canonical', action='store_true')
    ap.add_argument('--host-full', action='store_true')
    args = ap.parse_args()
    if args.build_canonical:
        return build_canonical()
    cost, cost_from = product_cost(args.detail)
    if not cost:                                                             # a headline-only bench run writes no second_roof table
        cost, cost_from = product_cost('')                                   # ... then the latest committed one (another session's)
    name = lambda c: str(c) if c < 1024 else f'2^{c.bit_length() - 1}'
    lines = ['# Rescue permutations and trees on the device (tools/rescue_bench.py)', '',
             '4 x 128 of examples/rescue: x^3 and its inverse, 32 rounds; the modified sponge of the tree (31 double rounds), two inputs, one element out.',
             'Time per launch: host clock around back-to-back launches ending in one synchronise, after a warm-up.',
             f'Product roof: per-product cost from `{cost_from}` (`second_roof`, canonical 128-bit product, ns per wave at the kernel\'s waves per SIMD) / 64 lanes / 1 024 SIMDs.'
             if cost else 'Product roof: no `second_roof` table was found: no fractions.', '']
    results = {}
    for label, lib_path in (('lazy chain (the library)', None), ('canonical chain (-DGS_RESCUE_CANONICAL_CHAIN)', CANONICAL_LIB)):
        if lib_path is not None and not os.path.exists(lib_path):
            lines += [f'## {label}', '', 'not measured: the library was not built (`tools/rescue_bench.py --build-canonical`).', '']
            continue
        be = Backend(device=0, lib_path=lib_path)
        f = PrimeField(backend=be)
        h = rescue4x128(f)
        series = f.getPowerSeries(3, (1 << 20) * 2)                          # inputs made on the device: distinct non-trivial elements
        src = Matrix(be, 1 << 20, 2, owner=series._owner)
        out = Matrix(be, 1 << 20, 1)
        per = products_per_permutation(be, h, src, out)
        roof = lambda count, form: count * per * cost[min(OCCUPANCY[form], 4) - 1] * 1e-9 / (LANES * SIMDS) if cost else None
        table = permutation_table(be, h, src, out, args.window, COUNTS, (1, 2), roof)
        results[label] = table
        lines += [f'## {label}: {per} products per permutation', '',
                  '| permutations | form | reps | ms per launch | k permutations/s | G products/s | fraction of product roof |', '|---|---|---|---|---|---|---|']
        for (count, form), (t, reps, r) in table.items():
            lines.append(f'| {name(count)} | {form} | {reps} | {t * 1e3:.4f} | {count / t / 1e3:.2f} | {count * per / t / 1e9:.2f} | {r / t:.3f} |' if r else
                         f'| {name(count)} | {form} | {reps} | {t * 1e3:.4f} | {count / t / 1e3:.2f} | {count * per / t / 1e9:.2f} | n/a |')
        lines.append('')
        if lib_path is None:
            limit = be.lib.gs_rescue_spread_limit()
            fine = [1 << k for k in range(10, 21)]
            cross = permutation_table(be, h, src, out, args.window / 4, fine, (1, 2), roof)
            lines += [f'Crossover of the forms (gs_rescue_spread_limit() = {name(limit)}; ms per launch):', '',
                      '| permutations | form 1 | form 2 |', '|---|---|---|']
            lines += [f'| {name(c)} | {cross[(c, 1)][0] * 1e3:.4f} | {cross[(c, 2)][0] * 1e3:.4f} |' for c in fine]
            lines.append('')
            lines += ['Trees (leaves in place, one launch per level, form chosen by the library):', '',
                      '| leaves | reps | ms | ms per level | fraction of product roof (form 1 occupancy) |', '|---|---|---|---|---|']
            nodes = Vector(be, 2 << 20)
            for log in (8, 16, 20):
                n = 1 << log
                be.call('gs_copy', C.c_void_p(nodes.ptr + n * f.elementSize), C.c_void_p(src.ptr), n * f.elementSize)
                t, reps = timed(be, lambda: be.call('gs_rescue_merkle', h.handle(), C.c_void_p(nodes.ptr + n * f.elementSize), n, C.c_void_p(nodes.ptr)), args.window)
                r = roof(n - 1, 1)
                results[('tree', log)] = t
                lines.append(f'| 2^{log} | {reps} | {t * 1e3:.3f} | {t * 1e3 / log:.3f} | {r / t:.3f} |' if r else f'| 2^{log} | {reps} | {t * 1e3:.3f} | {t * 1e3 / log:.3f} | n/a |')
            lines.append('')
        be.close()
    # the host-integer fallback of RescueMerkleTree (what a library without the entries gives), same machine, one core
    hf = HostField(MODULUS_128)
    hh = rescue4x128(hf)
    hh.keys                                                                  # (unrolled before the clock starts)
    leaves = [pow(3, i + 1, hf.modulus) for i in range(1 << (16 if args.host_full else 8))]
    t0 = time.perf_counter()
    RescueMerkleTree(hh, leaves[:256])
    host8 = time.perf_counter() - t0
    if args.host_full:
        t0 = time.perf_counter()
        RescueMerkleTree(hh, leaves)
        host16, how = time.perf_counter() - t0, 'run whole'
    else:
        host16, how = host8 / 255 * 65535, '65 535 x the time per hash of the 2^8-leaf run (the fallback is a plain loop over hash2)'
    lines += ['## Host-integer fallback (RescueMerkleTree on Python integers, one core, same machine)', '',
              '| leaves | host | device | ratio |', '|---|---|---|---|']
    for log, host, note in ((8, host8, 'run whole'), (16, host16, how)):
        dev = results.get(('tree', log))
        lines.append(f'| 2^{log} | {host:.2f} s ({note}) | {dev * 1e3:.3f} ms | {host / dev:.0f} x |' if dev else f'| 2^{log} | {host:.2f} s ({note}) | n/a | n/a |')
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
