"""csrc/air_codegen.h — the generator of compiled AIR programs, plain C++ — run where there is no GPU and no device library: a stand-alone
program built with g++ (tests/host_harness/air_codegen_host.cpp: all six fixed field flavours in one binary, also with
-fsanitize=address,undefined) writes the source of every program of tests/air_codegen_corpus.py, and every source must be the one
recorded in tests/golden/air_jit_sources.json (SHA-256 and lane count; tests/golden/make_air_jit_sources.py says where the record comes
from).  The malformed programs of tests/test_air_program_header.py go through the same builds: the validator refuses each, the
generator never sees one.  And the name a library gives a code object in the on-disk cache is the recorded one, so the caches machines
already hold stay valid."""
import ctypes as C
import json
import os
import subprocess

import pytest

import air_codegen_corpus as cc
from conftest import ROOT
from field_corners import FIXED
from genstark_amd._abi import HIP_LIB_PATHS
from test_air_program_header import CASES

SOURCE = os.path.join(ROOT, 'tests', 'host_harness', 'air_codegen_host.cpp')
with open(os.path.join(ROOT, 'tests', 'golden', 'air_jit_sources.json')) as _fh:
    GOLDEN = json.load(_fh)
_BUILT = {}


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    """sanitized or not -> the filter, built on first use (a program of its own: nothing is preloaded)."""
    def get(sanitized=False):
        if sanitized not in _BUILT:
            exe = str(tmp_path_factory.mktemp('air_codegen_host') / f'air_codegen_host{"_san" if sanitized else ""}')
            extra = ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] if sanitized else ['-O2']
            subprocess.check_call(['g++', '-std=c++17', '-Wall', *extra, SOURCE, '-o', exe])
            _BUILT[sanitized] = exe
        return _BUILT[sanitized]
    return get


def feed(exe, texts):
    r = subprocess.run([exe], input=''.join(texts), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, f'exit {r.returncode}:\n{r.stdout[-500:]}\n{r.stderr[-3000:]}'
    out = r.stdout.split('\n')
    assert len(out) == len(texts) + 1 and out[-1] == ''
    return out[:-1]


def test_golden_file_covers_the_corpus():
    assert list(GOLDEN) == cc.FLAVOUR_NAMES == ['p128', 'q64', 'q32', 'q17', 'p256', 'p224']
    for name in cc.FLAVOUR_NAMES:
        names = set(GOLDEN[name]['sources'])
        assert {f'generated_{seed}' for seed in cc.SEEDS} <= names and {'rows', 'lanes16', 'pow_groups', 'statics', 'init_seglen1'} <= names
        assert sum(n.startswith('constraints_') for n in names) == 24
    assert {'rescue4x128_segmented_trace', 'poseidon6x128_segmented_trace', 'poseidon6x128_segmented_constraints', 'rescue4x128_constraints'} <= set(GOLDEN['p128']['sources'])
    assert {'point_mul_trace', 'verify_schnorr_signature_trace', 'verify_schnorr_signature_constraints'} <= set(GOLDEN['p224']['sources'])


@pytest.mark.parametrize('sanitized', [False, True])
@pytest.mark.parametrize('name', cc.FLAVOUR_NAMES)
def test_generated_sources_equal_the_recorded_ones(name, sanitized, harness):
    entries = cc.corpus(name)
    want = GOLDEN[name]['sources']
    assert [e.name for e in entries] == list(want), 'the corpus and the golden file list the same programs in the same order'
    wrong = []
    for e, line in zip(entries, feed(harness(sanitized), [cc.harness_text(name, e) for e in entries])):
        expected = want[e.name] if want[e.name] == 'declined' else f'{want[e.name][0]} {want[e.name][1]}'
        if line != expected:
            wrong.append(f'{e.name}: {line} (recorded: {expected})')
    assert not wrong, '\n'.join(wrong)


@pytest.mark.parametrize('sanitized', [False, True])
def test_malformed_programs_never_reach_the_generator(sanitized, harness):
    """Every flavour, every malformed program of the header's table refused with the validator's message; every neighbour generates."""
    texts, cases = [], []
    for name in cc.FLAVOUR_NAMES:
        for c in CASES:
            e = cc._entry(c.name, c.kind, c.code, c.init, [5] * c.nconsts, c.vm_regs, c.registers, c.nout, [2] * c.nstatic,
                          [3, FIXED[name][0] - 1] * c.nstatic if c.kind == 'trace' and c.nstatic <= 64 else None)
            texts.append(cc.harness_text(name, e))
            cases.append((name, c))
    for (name, c), line in zip(cases, feed(harness(sanitized), texts)):
        if c.bad_at is None:
            assert len(line.split()) == 2 and len(line.split()[0]) == 64, f'{name} {c.name}: {line}'
        else:
            assert line.startswith('refused air program: '), f'{name} {c.name}: {line}'
            if c.bad_at != 'shape':
                assert f'invalid instruction {c.bad_at} (op ' in line, f'{name} {c.name}: {line}'


@pytest.mark.parametrize('name', cc.FLAVOUR_NAMES)
def test_cache_file_name_is_the_recorded_one(name, tmp_path, monkeypatch):
    """gs_jit_cache_path_probe: entry name, target, key version, the embedded field headers and the source, hashed as before."""
    cache = tmp_path / 'cache'
    monkeypatch.setenv('GSTARK_JIT_CACHE_DIR', str(cache))
    lib = C.CDLL(HIP_LIB_PATHS[FIXED[name][0]])
    buf = C.create_string_buffer(4096)
    assert lib.gs_jit_cache_path_probe(cc.CACHE_PROBE_SOURCE, buf, C.c_uint64(len(buf))) == 0
    assert buf.value.decode() == f'{cache}/{GOLDEN[name]["cache_file"]}'
