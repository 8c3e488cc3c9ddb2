"""Several prime fields in one node process (js/galois.js: one library object per field; napi/gstark_napi.cc: open(path)).
tests/js_multi_field.js proves statements over the 128-, 64-, 32- and 224-bit fields and a runtime-modulus prime, interleaved, member by
member and through the one-call entries, each proof verified natively; the same statements proved one per process (the single-field path:
GSTARK_LIB naming one library on the CPU tier) give the same bytes.  On the MI355X the same script runs on the HIP libraries at the anchored
sizes (MiMC-128 2^13 E = 8 is C2_E8, the ledger at 4 096 runs is X_shaped: tests/golden/config_digests.json)."""
import json
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT, _build_oracle

NODE = shutil.which('node')
HAVE_HEADERS = os.path.exists('/usr/include/node/node_api.h')
pytestmark = pytest.mark.skipif(not (NODE and HAVE_HEADERS), reason='node or its headers are not in this image')

SCRIPT = os.path.join(ROOT, 'tests', 'js_multi_field.js')
STATEMENTS = ['mimc128', 'ledger128', 'chain64', 'chain32', 'chain224', 'chainRuntime']
# the single-field path on the CPU tier: GSTARK_LIB names the one oracle library of the statement's field
ORACLE_FOR = {'mimc128': 'liboracle.so', 'ledger128': 'liboracle.so', 'chain64': 'liboracle_q64.so', 'chain32': 'liboracle_q32.so',
              'chain224': 'liboracle_p224.so', 'chainRuntime': 'liboracle_rt.so'}
DIGESTS = {r['name']: r for r in json.load(open(os.path.join(ROOT, 'tests', 'golden', 'config_digests.json')))}


@pytest.fixture(scope='module')
def addon():
    subprocess.check_call(['bash', os.path.join(ROOT, 'napi', 'build.sh')])
    return os.path.join(ROOT, 'napi', 'gstark_napi.node')


def run_script(env_extra, tier, seed, out, only=None, timeout=600):
    """one node process under a time limit of its own"""
    env = dict(os.environ, **env_extra)
    cmd = ['timeout', '-k', '10', str(timeout), NODE, SCRIPT, tier, str(seed), str(out)] + ([only] if only else [])
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout + 30)
    assert r.returncode == 0 and 'js multi-field OK' in r.stdout, (only, r.returncode, r.stderr[-3000:])
    return json.loads(out.read_text())


def check(interleaved, singles):
    assert interleaved.pop('_checks') == 'ok'
    assert sorted(interleaved) == sorted(STATEMENTS)
    assert len({r['modulus'] for r in interleaved.values()}) == 5
    for name in STATEMENTS:
        assert interleaved[name] == singles[name], name


def test_multi_field_interleaved_on_oracle_double(addon, tmp_path):
    _build_oracle()
    seed = random.randrange(1 << 30)
    lib_dir = {'GSTARK_LIB_DIR': os.path.join(ROOT, 'oracle'), 'GSTARK_ALLOW_TEST_DOUBLE': '1'}
    interleaved = run_script(lib_dir, 'small', seed, tmp_path / 'all.json')
    singles = {}
    for name in STATEMENTS:
        one = {'GSTARK_LIB': os.path.join(ROOT, 'oracle', ORACLE_FOR[name]), 'GSTARK_ALLOW_TEST_DOUBLE': '1'}
        if name == 'chainRuntime':
            one['GSTARK_SET_MODULUS'] = '1'
        singles[name] = run_script(one, 'small', seed, tmp_path / f'{name}.json', only=name)[name]
    check(interleaved, singles)


def test_addon_library_objects_refuse_malformed_calls(addon):
    env = dict(os.environ, GSTARK_ADDON=addon, GSTARK_LIB_DIR=os.path.join(ROOT, 'oracle'),
               GSTARK_PROVER_LIB=os.path.join(ROOT, 'genstark_amd', 'csrc', 'libgstark_prover.so'))
    _build_oracle()
    r = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'addon_library_validation.js')], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'addon library validation OK: 27 malformed calls refused' in r.stdout, r.stderr[-3000:]


def test_addon_library_objects_under_sanitizers():
    """the same malformed calls through the ASAN + UBSAN build of the addon (tools/build_sanitized.sh)"""
    import test_sanitizers as ts
    if not (ts.ASAN and ts.STDCPP):
        pytest.skip('libasan is not in this image')
    _build_oracle()
    sanitized = subprocess.check_output(['bash', os.path.join(ROOT, 'tools', 'build_sanitized.sh')], text=True).strip().splitlines()[-1]
    env = ts.san_env(sanitized, GSTARK_ADDON=os.path.join(sanitized, 'gstark_napi.node'), GSTARK_LIB_DIR=os.path.join(ROOT, 'oracle'),
                     GSTARK_PROVER_LIB=os.path.join(sanitized, 'libgstark_prover.so'))
    ts.run_clean([NODE, os.path.join(ROOT, 'tests', 'addon_library_validation.js')], env, 'addon library validation OK: 27 malformed calls refused')


@pytest.mark.gpu
def test_multi_field_interleaved_on_hip(addon, tmp_path):
    """five flavours' code objects, contexts and caches in one process on one MI355X: the interleaved bytes equal the single-field runs'
    and, where the statement is an anchored configuration, the committed digest"""
    seed = random.randrange(1 << 30)
    interleaved = run_script({}, 'anchored', seed, tmp_path / 'all.json', timeout=900)
    singles = {name: run_script({}, 'anchored', seed, tmp_path / f'{name}.json', only=name, timeout=600)[name] for name in STATEMENTS}
    anchors = {name: rec['anchor'] for name, rec in interleaved.items() if isinstance(rec, dict) and rec.get('anchor')}
    assert anchors == {'mimc128': 'C2_E8', 'ledger128': 'X_shaped'}
    for name, anchor in anchors.items():
        rec = interleaved[name]
        assert (rec['proofBytes'], rec['proofSha256']) == (DIGESTS[anchor]['proof_bytes'], DIGESTS[anchor]['proof_sha256']), name
    check(interleaved, singles)
