"""Inputs, host references and harness pieces shared by tests/test_hades.py and tests/test_rescue_hash.py.  Not a test module."""
import os
import shutil
import subprocess

import pytest

from genstark_amd import _abi
from genstark_amd._abi import Backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which('node')
HAVE_HEADERS = os.path.exists('/usr/include/node/node_api.h')
needs_node = pytest.mark.skipif(not (NODE and HAVE_HEADERS), reason='node or its headers are not in this image')
FLAVOURS = {'p128': None, 'p224': _abi.MODULUS_224, 'q64': _abi.MODULUS_64}


def flavour_fixture(*names):
    @pytest.fixture(scope='module', params=names or list(FLAVOURS))
    def flavour(request):
        be = Backend(device=0, modulus=FLAVOURS[request.param])
        yield be
        be.close()
    return flavour


def input_rows(rng, p, count, arity):
    """rows of `arity` inputs: 0, 1 and p - 1 in every position of the first rows, random elements after"""
    special = [[v] * arity for v in (0, 1, p - 1)] + [[(0, 1, p - 1)[(j + s) % 3] for j in range(arity)] for s in range(3)]
    return (special + [[rng.randrange(p) for _ in range(arity)] for _ in range(max(count - len(special), 0))])[:count]


def heap_nodes(leaves, node, unused):
    """the heap layout from host values: nodes[i] = node(nodes[2i], nodes[2i + 1]) above the leaves, `unused` at index 0"""
    n = len(leaves)
    nodes = [unused] * n + list(leaves)
    for i in range(n - 1, 0, -1):
        nodes[i] = node(nodes[2 * i], nodes[2 * i + 1])
    return nodes


def check_header_is_plain_c(family):
    r = subprocess.run(['gcc', '-fsyntax-only', '-x', 'c', '-std=c99', '-Wall', '-Werror', os.path.join(ROOT, 'include', f'gstark_{family}.h')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def check_symbol_table(family, symbols, other_tables):
    header = open(os.path.join(ROOT, 'include', f'gstark_{family}.h')).read()
    for name in symbols:
        assert name + '(' in header, name
    for table in other_tables:
        assert set(symbols).isdisjoint(table)
    assert f'gs_{family}' not in open(os.path.join(ROOT, 'include', 'gstark.h')).read()


def run_js(family, mode, tmp_path, expectations):
    """tests/js_<family>.js in `mode` ('hip', or 'double': the tests' double, which lacks the entry points) against what expectations(path) writes"""
    env_extra = {}
    if mode == 'double':
        from conftest import _build_oracle
        _build_oracle()
        env_extra = {'GSTARK_LIB_DIR': os.path.join(ROOT, 'oracle'), 'GSTARK_ALLOW_TEST_DOUBLE': '1'}
    subprocess.check_call(['bash', os.path.join(ROOT, 'napi', 'build.sh')], stdout=subprocess.DEVNULL)
    want = tmp_path / 'want.json'
    expectations(want)
    r = subprocess.run(['timeout', '-k', '10', '240', NODE, os.path.join(ROOT, 'tests', f'js_{family}.js'), mode, str(want)], cwd=ROOT,
                       env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'js {family} ({mode}) OK' in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
