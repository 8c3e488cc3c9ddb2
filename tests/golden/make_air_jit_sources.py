"""tests/golden/make_air_jit_sources.py — what tests/test_air_codegen_host.py compares the code generator (csrc/air_codegen.h) against:
per field flavour and program of tests/air_codegen_corpus.py, the SHA-256 of the HIP source a BUILT library generates and its lane
count ("declined" where the generator leaves a program to the interpreter), and the name of the cache file the library gives a fixed
probe source; writes tests/golden/air_jit_sources.json.

    python tests/golden/make_air_jit_sources.py <directory with libgstark_hip*.so>

The sources are taken where the library hands them to the compiler: gs_air_jit_check_statics with GSTARK_AIR_JIT_DUMP set.  The hook
also compiles each source, which takes hours over the whole corpus; a scratch build whose jit_compile returns right after the dump is
written records the same text in a minute.  The committed file was recorded that way from commit 406188b, the last one with the
generator inside air_jit.hip, so it pins the text as it was before the generator moved.  Run it again, on a library built from the
tree, only after a change of the generated text that is meant."""
import ctypes as C
import hashlib
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

LIBRARIES = {'p128': 'libgstark_hip.so', 'q64': 'libgstark_hip_q64.so', 'q32': 'libgstark_hip_q32.so', 'q17': 'libgstark_hip_q17.so',
             'p256': 'libgstark_hip_p256.so', 'p224': 'libgstark_hip_p224.so'}


def record(lib, entries, dump_dir):
    from air_codegen_corpus import through_hook
    out = {}
    for e in entries:
        before = set(os.listdir(dump_dir))
        rc, log = through_hook(lib, e)
        new = sorted(set(os.listdir(dump_dir)) - before)
        if not new:
            assert 'does not know' in log, f'{e.name}: no source and no refusal by the generator ({rc}: {log})'
            out[e.name] = 'declined'
            continue
        assert len(new) == 1, (e.name, new)
        with open(os.path.join(dump_dir, new[0]), 'rb') as fh:
            source = fh.read()
        lanes = re.search(rb'#define GS_LANES (\d+)u', source)
        out[e.name] = [hashlib.sha256(source).hexdigest(), int(lanes.group(1)) if lanes else 1]
    return out


def cache_name(lib, directory):
    from air_codegen_corpus import CACHE_PROBE_SOURCE
    os.environ['GSTARK_JIT_CACHE_DIR'] = directory
    buf = C.create_string_buffer(4096)
    assert lib.gs_jit_cache_path_probe(CACHE_PROBE_SOURCE, buf, C.c_uint64(len(buf))) == 0
    return os.path.basename(buf.value.decode())


if __name__ == '__main__':
    from air_codegen_corpus import FLAVOUR_NAMES, corpus
    golden = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in FLAVOUR_NAMES:
            dump_dir = os.path.join(tmp, name)          # one per library: each numbers its dumps from zero
            os.mkdir(dump_dir)
            os.environ['GSTARK_AIR_JIT_DUMP'] = dump_dir
            lib = C.CDLL(os.path.join(sys.argv[1], LIBRARIES[name]))
            golden[name] = {'cache_file': cache_name(lib, os.path.join(tmp, 'cache')), 'sources': record(lib, corpus(name), dump_dir)}
            print(name, len(golden[name]['sources']), 'programs', file=sys.stderr)
    with open(os.path.join(HERE, 'air_jit_sources.json'), 'w') as fh:
        json.dump(golden, fh, indent=0, separators=(',', ':'))
        fh.write('\n')
