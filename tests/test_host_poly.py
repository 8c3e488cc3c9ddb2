"""The HOST-side polynomial helpers of the library (csrc/host_poly.h: transform, product of linear factors, batch inversion, Horner),
the digest -> element and modulus helpers of csrc/host_field.h and the bigint -> bytes quirk of csrc/host_hash.h against Python
integers, without a GPU: the native drivers, the verifier and gs_small_interpolate all compute with these, and the other tiers only
see them through whole proofs.  tools/host_poly_check.cpp wraps them as a filter; it is built per field flavour, plainly and with
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone host program)."""
import hashlib
import os
import random
import subprocess

import pytest

from conftest import ROOT
from genstark_amd._abi import MODULUS_128, MODULUS_224, MODULUS_256, MODULUS_32, MODULUS_64

FLAVOURS = {'p128': (MODULUS_128, []), 'p224': (MODULUS_224, ['-DGS_WIDE_BITS=224']), 'p256': (MODULUS_256, ['-DGS_WIDE_BITS=256']),
            'q64': (MODULUS_64, [f'-DGS_SMALL_Q={MODULUS_64}ull']), 'q32': (MODULUS_32, [f'-DGS_SMALL_Q={MODULUS_32}ull'])}
BUILDS = {'plain': ['-O2'], 'sanitized': ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer']}


def _root_of_unity(p, n, rng):
    """An element of order exactly n (a power of two dividing p - 1)."""
    assert (p - 1) % n == 0
    while True:
        w = pow(rng.randrange(2, p), (p - 1) // n, p)
        if n == 1 or pow(w, n // 2, p) != 1:
            return w


def _cases(name, p):
    """[(command line, expected output tokens as integers or strings[, leading tokens to skip])] — one list for both builds of a flavour."""
    rng = random.Random(name)
    weak = name == 'p128'       # the only flavour with more than one representative of a value: v + p where it fits 128 bits
    spare = 2**128 - p if weak else 0

    def rep(v):                 # for helpers whose contract is "any representative"
        return v + p if v < spare and rng.random() < 0.5 else v

    def small_or_random():      # values that have a second 128-bit representative among uniform ones
        return rng.randrange(spare) if weak and rng.random() < 0.4 else rng.randrange(p)

    def line(cmd, *vals):
        return ' '.join([cmd] + [v if isinstance(v, str) else f'{v:064x}' for v in vals])

    cases = []
    # transform: against the naive sum, and forward-then-inverse = n a
    for n in (1, 2, 4, 8, 64, 128):
        w = _root_of_unity(p, n, rng)
        for edge in (False, True):
            a = [rng.choice((0, 1, p - 1)) for _ in range(n)] if edge else [small_or_random() for _ in range(n)]
            fwd = [sum(a[i] * pow(w, i * j, p) for i in range(n)) % p for j in range(n)]
            cases.append((line('T', str(n), w, pow(w, p - 2, p), *[rep(v) for v in a]), fwd + [n * v % p for v in a]))
    # product of linear factors (64 | 65: the verifier's schoolbook limit); repeated points and the point 0
    for m in (0, 1, 2, 3, 64, 65):
        for variant in range(3):
            xs = [rng.randrange(p) for _ in range(m)]
            if variant == 1 and m:
                xs[0] = 0
                xs[-1] = 0 if m > 2 else xs[-1]
            if variant == 2 and m > 1:
                xs[1:] = [xs[0]] * (m - 1) if m <= 3 else xs[1:m // 2] + xs[1:m - m // 2 + 1]
                xs[-1] = p - 1
            assert len(xs) == m
            zp = [1]
            for x in xs:
                zp = [((zp[d - 1] if d else 0) - x * (zp[d] if d < len(zp) else 0)) % p for d in range(len(zp) + 1)]
            cases.append((line('L', str(m), *xs), zp))
    # batch inversion: 0 stays 0 — first, last, everywhere
    for v in ([], [0], [rng.randrange(1, p)], [p - 1], [0] * 5, [0] + [rng.randrange(1, p) for _ in range(4)],
              [rng.randrange(1, p) for _ in range(4)] + [0], [0, 1, 0, p - 1, 0], [rng.randrange(1, p) for _ in range(5)]):
        cases.append((line('I', str(len(v)), *v), [pow(x, p - 2, p) for x in v]))
    # horner / horner_many: empty, constant, x = 0, x = p - 1
    for n in (0, 1, 2, 7, 40):
        poly = [small_or_random() for _ in range(n)]
        xs = [0, p - 1, 1, rng.randrange(p), small_or_random()]
        want = [sum(c * pow(x, k, p) for k, c in enumerate(poly)) % p for x in xs]
        cases.append((line('H', str(n), *poly, str(len(xs)), *xs), want + want))        # canonical operands: both forms
        if weak:                # horner_many takes any representative of coefficients and points; horner's half of the line is skipped
            cases.append((line('H', str(n), *[rep(v) for v in poly], str(len(xs)), *[rep(x) for x in xs]), want, len(xs)))
    # hf_from_digest: the 256-bit big-endian integer mod p
    for v in (0, 2**256 - 1, p - 1, p, p + 1, 2**255, 2**128, 2**128 - 1, rng.randrange(2**256)):
        cases.append((line('D', f'{v:064x}'), [v % p]))
    for msg in (b'', b'abc', b'genstark', bytes(range(200))):
        cases.append((line('S', msg.hex() or '-'), [int.from_bytes(hashlib.sha256(msg).digest(), 'big') % p]))
    cases.append((line('P'), [p]))
    # host_bigint_bytes: Buffer.from(v.toString(16), 'hex') — an odd digit count loses the last nibble
    for v, width in ((0, 33), (0, 1), (1, 33), (0xabc, 33), (0xabcd, 33), (2**256 + 5, 33), (2**260 - 1, 33), (2**263 + 0x1234, 33),
                     (rng.randrange(2**255, 2**256), 33), (rng.randrange(2**248, 2**252), 33), (rng.randrange(2**120), 33),
                     (rng.randrange(2**255, 2**256), 32), (rng.randrange(2**244, 2**248), 32)):
        digits = f'{v:x}' if v else ''
        cases.append((line('B', v.to_bytes(width, 'big').hex()), [digits[:len(digits) // 2 * 2] or '-']))
    return cases


_case_cache = {}


@pytest.mark.parametrize('build', sorted(BUILDS))
@pytest.mark.parametrize('name', sorted(FLAVOURS))
def test_host_poly_helpers(name, build, tmp_path):
    p, flags = FLAVOURS[name]
    exe = str(tmp_path / f'host_poly_check_{name}_{build}')
    subprocess.check_call(['g++', *BUILDS[build], '-std=c++17', '-Wall', '-Wno-unknown-pragmas', *flags, os.path.join(ROOT, 'tools', 'host_poly_check.cpp'), '-o', exe])
    if name not in _case_cache:
        _case_cache[name] = _cases(name, p)
    cases = _case_cache[name]
    text = ''.join(case[0] + '\n' for case in cases)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    out = run.stdout.split('\n')
    assert len(out) >= len(cases)
    for (cmd, want, *skip), got in zip(cases, out):
        got = got.split()[skip[0] if skip else 0:]
        if cmd[0] == 'B':
            assert got == want, (name, cmd)
        else:
            assert [int(v, 16) for v in got] == want, (name, cmd[:200])
