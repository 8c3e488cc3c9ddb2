"""gs_prover_verify_device (include/gstark_prover.h): the native verifier with the device's help for the long polynomials of a
statement — the same decision, error code and message as gs_prover_verify on every input.

GPU tier: the committed 5 000-assertion proof; statements proved here with the device providers forced at small sizes
(gs_prover_verify_device_min(1, 1)) against the host entry over seeded corruptions; public input-register columns; three more field
flavours; the Python and node surfaces.  CPU tier: bound to the oracle double (neither optional entry) the device entry answers with
the host providers; a null context is GS_ERR_ARG.
`python tests/test_verify_device.py runtime <q>` is the flavour check for the runtime-modulus build (one modulus per process)."""
import json
import os
import random
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

from genstark_amd import _abi
from genstark_amd._abi import Backend, GstarkError
from genstark_amd.errors import StarkError
from genstark_amd.field import PrimeField
from genstark_amd.native import NativeProver

from boundary_common import GOLDEN, OPTS, Statement, golden_statement, quintic_air, quintic_trace, rescue_statement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def verdict(nat, assertions, data, public=None, device=False):
    """('ok', '') or (the exception's class, its whole text: the driver's code and message)"""
    try:
        return ('ok', '') if nat.verify_bytes(assertions, data, public, device=device) is True else ('false', '')
    except (StarkError, GstarkError) as e:
        return (type(e).__name__, str(e))


def corruptions(data, count, seed):
    """byte flips (three in four) and truncations, seeded"""
    rng = random.Random(seed)
    for i in range(count):
        b = bytearray(data)
        if i % 4 == 3:
            del b[rng.randrange(len(b)):]
        else:
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        yield bytes(b)


def agree_on_corruptions(nat, assertions, data, count, seed, public=None, least=None):
    """both entries on `count` corrupted proofs: the same verdict and text for every one; -> how many were rejections"""
    rejected = 0
    for bad in corruptions(data, count, seed):
        host, dev = verdict(nat, assertions, bad, public), verdict(nat, assertions, bad, public, device=True)
        assert host == dev, (host, dev)
        rejected += host[0] != 'ok'
    if least is not None:
        assert rejected >= least, f'{rejected} of {count} corruptions were rejected: the agreement is not about rejections'
    return rejected


class forced:
    """the device providers for every register with two or more assertions and every column of period two or more"""

    def __init__(self, nat):
        self.nat = nat

    def __enter__(self):
        self.nat.verify_device_min(1, 1)

    def __exit__(self, *exc):
        self.nat.verify_device_min(0, 0)


def quintic_statement(f, steps, ms, seed=1):
    rows = quintic_trace(f.modulus, steps, [5, 9])
    rng = random.Random(seed)
    a = []
    for reg, m in enumerate(ms):
        a += [{'step': s, 'register': reg, 'value': rows[s][reg]} for s in rng.sample(range(steps), m)]
    rng.shuffle(a)
    return quintic_air(f, steps), a, [5, 9]


def accept_and_reject(nat, a, data, public=None):
    """one accept and one reject case through both entries"""
    assert verdict(nat, a, data, public) == verdict(nat, a, data, public, device=True) == ('ok', '')
    wrong = [dict(x) for x in a]
    wrong[len(a) // 2]['value'] = (wrong[len(a) // 2]['value'] + 1) % nat.field.modulus
    host, dev = verdict(nat, wrong, data, public), verdict(nat, wrong, data, public, device=True)
    assert host == dev and host[0] == 'StarkError' and 'linear combination correctness' in host[1], (host, dev)


# ---------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_golden_proof_with_5000_assertions(hip_backend):
    """tests/golden/many_assertions_quintic_2p13.proof (tools/make_many_assertions_golden.py): above any threshold, no proving needed"""
    f = PrimeField(backend=hip_backend)
    nat = NativeProver(Statement(quintic_air(f, 1 << 13)))
    a = golden_statement(f.modulus)
    data = open(GOLDEN, 'rb').read()
    assert nat.verify_bytes(a, data, device=True) is True
    accept_and_reject(nat, a, data)
    # a repeated cell is refused by both with the host form's words, before any device work
    host, dev = verdict(nat, a + [a[10]], data), verdict(nat, a + [a[10]], data, device=True)
    assert host == dev and 'asserted more than once' in host[1]
    agree_on_corruptions(nat, a, data, 8, 5000, least=8)


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['quintic', 'rescue'])
def test_boundary_providers_forced(hip_backend, which):
    """quintic AIR, 2^10 steps, 300 + 3 assertions; Rescue 4x128, 2^10 steps, 4 x 64 assertions: every asserted register's I_r, Z_r from
    the device; both entries accept, and agree on 200 corruptions of which at least 190 are rejections"""
    f = PrimeField(backend=hip_backend)
    if which == 'quintic':
        air, a, seed = quintic_statement(f, 1 << 10, (300, 3))
        nat = NativeProver(Statement(air))
    else:
        air, a, seed = rescue_statement(f, 32)
        assert len(a) == 4 * 64
        nat = NativeProver(Statement(air, dict(OPTS, exeQueryCount=68, friQueryCount=24)))
    data = nat.prove_bytes(a, [], seed)
    with forced(nat):
        accept_and_reject(nat, a, data)
        agree_on_corruptions(nat, a, data, 200, len(a), least=190)
    accept_and_reject(nat, a, data)                      # ... and at the default thresholds


@pytest.mark.gpu
def test_public_input_register_columns(hip_backend):
    """tests/golden/aa/ledger.aa, 4 runs (two secret input registers, one public nested under the first): the public register's column
    goes through the device; the honest proof, a changed public value and altered shapes get the same answers"""
    from genstark_amd import airassembly
    from genstark_amd.prover import Prover
    from test_airassembly import AA, ledger_model
    f = PrimeField(backend=hip_backend)
    runs = 4
    balances, factors = [100 + 7 * i for i in range(runs)], [3 + i for i in range(runs)]
    deposits = [[5 + i + 2 * j for j in range(4)] for i in range(runs)]
    model = ledger_model(f.modulus, balances, factors, deposits)
    last = 8 * runs - 1
    a = [{'step': 0, 'register': 0, 'value': balances[0]}, {'step': last, 'register': 2, 'value': model[last][2]}]
    air = airassembly.AssemblyAir(open(os.path.join(AA, 'ledger.aa')).read(), 'default', None, f)
    nat = Prover(air, {'hashAlgorithm': 'sha256', 'exeQueryCount': 24, 'friQueryCount': 12})._native
    data = nat.prove_bytes(a, [balances, factors, deposits], None)
    with forced(nat):
        assert verdict(nat, a, data, [deposits]) == verdict(nat, a, data, [deposits], device=True) == ('ok', '')
        other = [list(d) for d in deposits]
        other[0][1] += 1
        for public in ([other], [], [deposits[:-1]]):
            host, dev = verdict(nat, a, data, public), verdict(nat, a, data, public, device=True)
            assert host == dev and host[0] == 'StarkError', (host, dev)
        shapes = 1 + (1 + 4) + (1 + 4) + (1 + 8)         # the serialized iShapes are the proof's last bytes
        for k in range(1, shapes + 1):
            bad = bytearray(data)
            bad[-k] ^= 1
            host, dev = verdict(nat, a, bytes(bad), [deposits]), verdict(nat, a, bytes(bad), [deposits], device=True)
            assert host == dev and host[0] == 'StarkError', (k, host, dev)
        agree_on_corruptions(nat, a, data, 40, 4, public=[deposits], least=36)


def flavour_case(be):
    f = PrimeField(backend=be)
    air, a, seed = quintic_statement(f, 1 << 10, (300, 3), seed=f.modulus % 1009)
    nat = NativeProver(Statement(air))
    data = nat.prove_bytes(a, [], seed)
    with forced(nat):
        accept_and_reject(nat, a, data)
    accept_and_reject(nat, a, data)


@pytest.mark.gpu
@pytest.mark.parametrize('modulus', [_abi.MODULUS_64, _abi.MODULUS_224], ids=['q64', 'p224'])
def test_other_flavours(modulus):
    be = Backend(device=0, modulus=modulus)
    try:
        flavour_case(be)
    finally:
        be.close()


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    import subprocess
    from test_runtime_modulus import PRIMES
    q = PRIMES[6]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime verify_device: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_python_surface(hip_backend):
    """Prover.verify / verify_native / NativeProver.verify take device=: the same True, the same error text"""
    from genstark_amd.prover import Prover
    f = PrimeField(backend=hip_backend)
    air, a, seed = quintic_statement(f, 1 << 10, (300, 3))
    p = Prover(air, OPTS)
    data = p.prove_bytes(a, [], seed)
    assert p.verify(a, data) is True and p.verify(a, data, device=True) is True
    assert p.verify(a, p.parse(data), device=True) is True                     # a parsed proof is serialized again
    assert p.verify_native(a, data, device=True) is True and p._native.verify(a, data, device=True) is True
    wrong = [dict(a[0], value=a[0]['value'] ^ 1)] + a[1:]
    texts = []
    for device in (False, True):
        with pytest.raises(StarkError) as e:
            p.verify_native(wrong, data, device=device)
        texts.append(str(e.value))
    assert texts[0] == texts[1] and 'linear combination correctness' in texts[0]
    with pytest.raises(StarkError) as e:
        p.verify(wrong, data, device=True)
    assert str(e.value) == texts[0]


@pytest.mark.gpu
def test_js_verify_device(tmp_path):
    """js/prover.js: verifyGenericSerialized(..., {device: true}) equals the default on the committed golden proof"""
    import shutil
    import subprocess
    from genstark_amd.hostfield import HostField
    node = shutil.which('node')
    if not (node and os.path.exists('/usr/include/node/node_api.h')):
        pytest.skip('node or its headers are not in this image')
    subprocess.check_call(['bash', os.path.join(ROOT, 'napi', 'build.sh')], stdout=subprocess.DEVNULL)
    air = quintic_air(HostField(_abi.MODULUS_128), 1 << 13)
    case = {'generic': air.descriptor(), 'options': OPTS, 'proof': GOLDEN,
            'assertions': [dict(x, value=str(x['value'])) for x in golden_statement(_abi.MODULUS_128)]}
    (tmp_path / 'case.json').write_text(json.dumps(case))
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_verify_device.js'), str(tmp_path / 'case.json')], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'js verify device OK' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---------------------------------------------------------------------------------------------------------------- CPU tier
def _oracle_case(oracle_backend):
    import genstark_amd as ga
    with open(os.path.join(ROOT, 'tests', 'golden', 'oracle_proofs.json')) as fh:
        case = json.load(fh)[0]
    options = {'hashAlgorithm': case['hash_algorithm'], 'extensionFactor': case['extension_factor'], 'exeQueryCount': case['exe_query_count'],
               'friQueryCount': case['fri_query_count']}
    stark = ga.instantiateMimc(case['steps'], options, None, backend=oracle_backend)
    a = [{'step': x['step'], 'register': x['register'], 'value': int(x['value'])} for x in case['assertions']]
    return NativeProver(stark), a, bytes.fromhex(case['proofHex'])


def test_falls_back_on_a_library_without_the_optional_entries(oracle_backend):
    """the oracle double exports neither gs_boundary_polys nor gs_eval_polys_at_points: the device entry runs the host providers"""
    assert not hasattr(oracle_backend.lib, 'gs_boundary_polys') and not hasattr(oracle_backend.lib, 'gs_eval_polys_at_points')
    nat, a, data = _oracle_case(oracle_backend)
    with forced(nat):
        assert verdict(nat, a, data) == verdict(nat, a, data, device=True) == ('ok', '')
        assert agree_on_corruptions(nat, a, data, 50, 50) >= 45
    # ... also for the statement whose boundary values WOULD go to the device: 5 000 assertions through the host tree form
    f = PrimeField(backend=oracle_backend)
    nat = NativeProver(Statement(quintic_air(f, 1 << 13)))
    a = golden_statement(f.modulus)
    assert verdict(nat, a, open(GOLDEN, 'rb').read(), device=True) == ('ok', '')


def test_null_context_is_an_argument_error(oracle_backend):
    nat, a, data = _oracle_case(oracle_backend)

    class _NoContext:
        ctx = None
    backend, nat.backend = nat.backend, _NoContext()
    try:
        with pytest.raises(StarkError, match=r'verification failed \(-1\)'):           # GS_ERR_ARG, no message
            nat.verify_bytes(a, data, device=True)
        assert nat.verify_bytes(a, data) is True                                        # the host entry takes no context
    finally:
        nat.backend = backend


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    flavour_case(be)
    print(f'runtime verify_device: modulus {q} ok')
