"""csrc/gf128.h: sums of 256-bit products reduced once (fe_wide_add + fe_reduce_wide9 — what the table-reading MiMC composition pass
ends with), compiled for the host with both compilers and compared with Python integers.  Runs without a GPU."""
import ctypes
import os
import subprocess

import pytest

from conftest import P, ROOT, from_bytes, rand_elements, to_bytes

CLANG = '/opt/rocm/lib/llvm/bin/clang++'
TOP_LIMIT = 1 << 24          # fe_reduce_wide9 takes a ninth limb below this


@pytest.fixture(scope='module', params=['g++', CLANG])
def lib(request, tmp_path_factory):
    compiler = request.param
    if compiler != 'g++' and not os.path.exists(compiler):
        pytest.skip('ROCm clang not present')
    so = str(tmp_path_factory.mktemp('wide') / 'gf128_wide_sum_host.so')
    subprocess.check_call([compiler, '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'host_harness', 'gf128_wide_sum_host.cpp')])
    return ctypes.CDLL(so)


def dot(lib, rows):
    """rows: [(a0, b0, a1, b1, ...)] all with the same number of terms"""
    terms = len(rows[0]) // 2
    out = ctypes.create_string_buffer(16 * len(rows))
    lib.h_dot(to_bytes(v for r in rows for v in r[0::2]), to_bytes(v for r in rows for v in r[1::2]), out, len(rows), terms)
    return from_bytes(out.raw)


@pytest.mark.parametrize('terms', [1, 2, 3])
def test_sum_of_products_reduced_once(lib, rng, terms):
    n = 4000
    rows = [tuple(rand_elements(rng, 2 * terms, edge=0.3)) for _ in range(n)]
    rows += [(P - 1,) * (2 * terms), (0,) * (2 * terms), (P - 1, 1) * terms, (2**127,) * (2 * terms)]       # the largest sums: top = terms - 1
    # sums whose residue is tiny or just below p: the carry out of the second fold, and the closing subtraction of p
    inv = lambda v: pow(v, P - 2, P)
    for r in list(range(0, 12)) + [9 * 2**32 - 2, 9 * 2**32 - 1, 9 * 2**32, 2**64, 2**96 - 1, P - 1, P - 2, P - 9 * 2**32, P - 9 * 2**32 + 1]:
        for _ in range(8):
            head = [rng.randrange(1, P) for _ in range(2 * terms - 1)]
            rest = sum(head[2 * k] * head[2 * k + 1] for k in range(terms - 1))
            rows.append(tuple(head) + ((r - rest) * inv(head[-1]) % P,))
    want = [sum(r[2 * k] * r[2 * k + 1] for k in range(terms)) % P for r in rows]
    assert dot(lib, rows) == want


def test_reduce_with_a_ninth_limb(lib, rng):
    xs, tops = [], []
    for top in [0, 1, 2, 3, 255, TOP_LIMIT - 1] + [rng.randrange(TOP_LIMIT) for _ in range(200)]:
        for x in [0, 1, 2**256 - 1, 2**128 - 1, 2**128, P * P, P * P - 1, (2**128 - 1) << 128] + [rng.randrange(2**256) for _ in range(20)]:
            xs.append(x)
            tops.append(top)
        # residues around 0 and p again, now with the ninth limb in play
        for r in (0, 1, 9 * 2**32 - 1, P - 1):
            m = rng.randrange(1 << 100)
            x = (r + m * P - top * 2**256) % P
            x += P * rng.randrange((2**256 - x) // P)
            xs.append(x)
            tops.append(top)
    out = ctypes.create_string_buffer(16 * len(xs))
    lib.h_reduce9(b''.join(x.to_bytes(32, 'little') for x in xs), (ctypes.c_uint32 * len(tops))(*tops), out, len(xs))
    assert from_bytes(out.raw) == [(x + t * 2**256) % P for x, t in zip(xs, tops)]
