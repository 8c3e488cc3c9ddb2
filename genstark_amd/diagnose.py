"""genstark_amd.diagnose — why a statement does not prove (include/gstark_diagnose.h; csrc/diagnose.h, csrc/diagnose.hip).

    d = Prover(air, options).diagnose(assertions, inputs, seed)      # the arguments of prove(); no proof is made
    d.ok            # True: every assertion holds, every constraint holds on every step, every degree fits its declaration
    print(d)        # one line per finding, e.g.  constraint 1: declared degree 1 allows degree 62, measured 63: declare 2

prove() ends such a statement with "Low degree proof failed: Remainder is not a valid degree ... polynomial" whatever the cause; the three
causes — a wrong witness or assertion, an `evaluation` that drifted from its `transition`, an under-declared `constraintDegrees` entry —
show in different places, and the diagnosis looks at each (which also states the reference's degree rule).
"""


class Diagnosis:
    """assertions:  [{index, step, register, expected, found}] — every assertion the trace does not meet
    constraints: [{index, violations, firstStep, lastStep, firstValue, degree, declared, limit, needed, atLeast, allZero}], one per
                 constraint (none for the MiMC AIR, whose transition and constraint are both the library's).  violations counts the steps
                 [0, steps - 1) at which the constraint is not zero (firstStep = lastStep = steps - 1 when there is none; firstValue is what
                 it evaluates to at firstStep); degree is the measured degree of the constraint over the trace polynomials, limit the highest
                 degree its declared degree lets through, needed the smallest declaration the measured degree fits (a lower bound when
                 atLeast)."""

    def __init__(self, steps, assertions, constraints):
        self.steps, self.assertions, self.constraints = steps, assertions, constraints

    @property
    def ok(self):
        return not self.assertions and all(c['violations'] == 0 and (c['allZero'] or c['degree'] <= c['limit']) for c in self.constraints)

    def findings(self):
        out = []
        for a in self.assertions:
            out.append(f"assertion {a['index']}: step {a['step']}, register {a['register']} holds {a['found']}, not {a['expected']}")
        for c in self.constraints:
            if c['violations']:
                out.append(f"constraint {c['index']}: violated on {c['violations']} of {self.steps - 1} steps, first at step {c['firstStep']} "
                           f"(value {c['firstValue']}), last at step {c['lastStep']}")
            elif not c['allZero'] and c['degree'] > c['limit']:
                out.append(f"constraint {c['index']}: declared degree {c['declared']} allows degree {c['limit']}, measured "
                           f"{'at least ' if c['atLeast'] else ''}{c['degree']}: declare {'at least ' if c['atLeast'] else ''}{c['needed']}")
        return out

    def __str__(self):
        return '\n'.join(self.findings()) or 'ok'

    def __repr__(self):
        return f'Diagnosis(ok={self.ok}, assertions={self.assertions!r}, constraints={self.constraints!r})'


def from_native(raw, assertions, modulus):
    """NativeProver.diagnose's report + the assertions it was given -> Diagnosis"""
    found = [{'index': a['index'], 'step': assertions[a['index']]['step'], 'register': assertions[a['index']]['register'],
              'expected': assertions[a['index']]['value'] % modulus, 'found': a['found']} for a in raw['assertions']]
    return Diagnosis(raw['steps'], found, raw['constraints'])
