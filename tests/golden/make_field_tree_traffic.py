"""tests/golden/make_field_tree_traffic.py — what test_field_tree_matches_the_recorded_parent (tests/test_tree_update.py) compares the
tree entries against: for the 128-bit flavour and q64, the traffic tally and every value read back over field_tree_sequence of that
module; writes tests/golden/field_tree_traffic.json.  It needs a device.

    python tests/golden/make_field_tree_traffic.py

The committed file was recorded from commit 1795091, the last one with the family-neutral tree kernels and entries inside hades.hip
and the two batch drivers as header templates, so it pins launches and values as they were before that code moved to field_tree.hip.
Run it again, on a library built from the tree, only after a change of a launch, a traffic line or a value that is meant."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

if __name__ == '__main__':
    from genstark_amd._abi import Backend
    from test_tree_update import FIELD_TREE_FLAVOURS, FIELD_TREE_PIN, field_tree_sequence
    golden = {}
    for name, modulus in sorted(FIELD_TREE_FLAVOURS.items()):
        be = Backend(device=0, modulus=modulus) if modulus else Backend(device=0)
        try:
            golden[name] = field_tree_sequence(be)
        finally:
            be.close()
        print(name, {family: sum(e['launches'] for e in rec['traffic'].values()) for family, rec in golden[name].items()}, 'launches', file=sys.stderr)
    with open(sys.argv[1] if len(sys.argv) > 1 else FIELD_TREE_PIN, 'w') as fh:
        json.dump(golden, fh, indent=0, separators=(',', ':'), sort_keys=True)
        fh.write('\n')
