"""Host mirror of the `@guildofweavers/galois` surface genSTARK calls (FiniteField / Vector / Matrix).

Member names and argument meaning follow the TypeScript interface so that the callers
(genstark_amd/stark.py, genstark_amd/components/*.py — mirrors of lib/Stark.ts and
lib/components/*.ts) read like the reference.  Vectors and matrices are device-resident; every
vector/matrix/polynomial operation is one call into the C ABI (include/gstark.h -> HIP kernels).
Scalar (single bigint) operations and Lagrange interpolation of a handful of points are host
integer arithmetic, exactly as in the reference's JS layer.

Call sites of every member: SURVEY.md section 8(b).
"""
import ctypes as C
import hashlib
import weakref
from hashlib import sha256 as _sha256

from ._abi import Backend, GstarkError

ELEMENT_SIZE = 16
MODULUS = 2**128 - 9 * 2**32 + 1


def _le(v):
    return int(v).to_bytes(ELEMENT_SIZE, 'little')


def sha256_bigint(value):
    """galois utils.sha256 (same helper as lib/components/QueryIndexGenerator.ts:61-67): a bigint is
    hashed as Buffer.from(value.toString(16), 'hex') — no leading zeros, odd trailing nibble dropped."""
    if isinstance(value, int):
        nhex = (value.bit_length() + 3) >> 2
        if nhex & 1:
            value >>= 4                  # odd number of hex digits: Buffer.from(..., 'hex') drops the last nibble
        value = value.to_bytes(nhex >> 1, 'big')
    return int.from_bytes(_sha256(value).digest(), 'big')


# ---- the quadratic definitions on host integers: what the members of include/gstark_poly.h compute on a library without the entries
def _host_mul_linear(poly, x, p):
    """poly * (X - x)"""
    out = [0] * (len(poly) + 1)
    for k, c in enumerate(poly):
        out[k + 1] = (out[k + 1] + c) % p
        out[k] = (out[k] - c * x) % p
    return out


def _host_divmod(a, b, p):
    la, lb = len(a), len(b)
    if la < lb:
        return [0], (list(a) + [0] * lb)[:lb - 1]
    inv, r, q = pow(b[-1], -1, p), list(a), [0] * (la - lb + 1)
    for k in range(la - lb, -1, -1):
        q[k] = r[k + lb - 1] * inv % p
        if q[k]:
            for j in range(lb):
                r[k + j] = (r[k + j] - q[k] * b[j]) % p
    return q, r[:lb - 1]


def _host_eval(poly, xs, p):
    out = []
    for x in xs:
        acc = 0
        for c in reversed(poly):
            acc = (acc * x + c) % p
        out.append(acc)
    return out


def _host_interpolate(xs, ys, p):
    """sum_i y_i / M'(x_i) * M / (X - x_i), M = prod (X - x_i)"""
    m = [1]
    for x in xs:
        m = _host_mul_linear(m, x, p)
    out = [0] * len(xs)
    for x, y in zip(xs, ys):
        q, acc = [0] * len(xs), 0                # M / (X - x) by synthetic division, and its value at x: M'(x)
        for k in range(len(xs), 0, -1):
            acc = (m[k] + acc * x) % p
            q[k - 1] = acc
        w = y * pow(_host_eval(q, [x], p)[0], -1, p) % p
        for k, c in enumerate(q):
            out[k] = (out[k] + w * c) % p
    return out


_SQRT_SPLITS = {}


def host_two_adicity(p):
    """s of p - 1 = 2^s * t, t odd"""
    return ((p - 1) & -(p - 1)).bit_length() - 1


def host_sqrt(a, p):
    """The even one of the two square roots of a modulo the prime p, or None (Tonelli-Shanks on host integers: the answer of
    gs_field_sqrt, include/gstark_sqrt.h, where a library lacks it; 0 is a square with root 0)."""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    if p not in _SQRT_SPLITS:
        s = host_two_adicity(p)
        z = next((z for z in range(2, 1000) if pow(z, (p - 1) // 2, p) == p - 1), None)
        if z is None:
            raise GstarkError(f'sqrt: modulus is not prime ({p})')
        _SQRT_SPLITS[p] = (s, (p - 1) >> s, pow(z, (p - 1) >> s, p))
    s, t, c = _SQRT_SPLITS[p]
    r, b, m = pow(a, (t + 1) // 2, p), pow(a, t, p), s
    while b != 1:
        i, sq = 0, b
        while sq != 1:
            sq, i = sq * sq % p, i + 1
            if i == m:
                raise GstarkError(f'sqrt: modulus is not prime ({p})')
        f = pow(c, 1 << (m - i - 1), p)
        r, c = r * f % p, f * f % p
        b, m = b * c % p, i
    return r if r % 2 == 0 else p - r


class _DeviceBuffer:
    """Owns one gs_alloc'd range; freed when the last Vector/Matrix viewing it is collected."""

    def __init__(self, backend, nbytes):
        self.backend, self.nbytes = backend, nbytes
        self.ptr = backend.alloc(max(nbytes, 16))

    def __del__(self):
        try:
            if self.ptr:
                self.backend.free(self.ptr)
                self.ptr = 0
        except Exception:
            pass


class Vector:
    """galois Vector: `length` elements of `elementSize` bytes, little-endian."""

    def __init__(self, backend, length, owner=None, offset=0, element_size=None):
        element_size = element_size or backend.element_size          # 16; 32 in the 256- / 224-bit library flavours
        self.backend, self.length, self.elementSize = backend, int(length), element_size
        self._owner = owner or _DeviceBuffer(backend, self.length * element_size)
        self._offset = offset
        self.series_base = None  # set when the vector is known to be {base^i}: lets NTT calls skip a readback

    @property
    def ptr(self):
        return self._owner.ptr + self._offset

    @property
    def byteLength(self):
        return self.length * self.elementSize

    def getValue(self, index):
        return int.from_bytes(self.backend.download(self.ptr, self.elementSize, index * self.elementSize), 'little')

    def toValues(self):
        raw = self.toBuffer()
        es = self.elementSize
        return [int.from_bytes(raw[i * es:(i + 1) * es], 'little') for i in range(self.length)]

    def toBuffer(self, start=0, count=None):
        count = self.length - start if count is None else count
        return self.backend.download(self.ptr, count * self.elementSize, start * self.elementSize)

    def copyValue(self, index, destination, offset):
        """lib/Stark.ts:290 — writes element `index` into `destination` (bytearray), returns bytes written."""
        destination[offset:offset + self.elementSize] = self.backend.download(
            self.ptr, self.elementSize, index * self.elementSize)
        return self.elementSize

    def valuesAt(self, indexes):
        """Batched copyValue: the raw bytes of the elements at `indexes` (one device gather)."""
        return self.backend.gather(self.ptr, self.elementSize, list(indexes))


class Matrix:
    """galois Matrix: rowCount x colCount elements, row-major contiguous (LowDegreeProver.ts:45)."""

    def __init__(self, backend, rows, cols, owner=None, offset=0):
        self.backend, self.rowCount, self.colCount, self.elementSize = backend, int(rows), int(cols), backend.element_size
        self._owner = owner or _DeviceBuffer(backend, self.rowCount * self.colCount * self.elementSize)
        self._offset = offset
        self.quartic_domain = None  # (omega, n, step) when built by transposeVector(power series, 4, step)

    @property
    def ptr(self):
        return self._owner.ptr + self._offset

    def getValue(self, row, col):
        off = (row * self.colCount + col) * self.elementSize
        return int.from_bytes(self.backend.download(self.ptr, self.elementSize, off), 'little')

    def toValues(self):
        raw = self.toBuffer()
        c, es = self.colCount, self.elementSize
        return [[int.from_bytes(raw[(r * c + k) * es:(r * c + k + 1) * es], 'little') for k in range(c)]
                for r in range(self.rowCount)]

    def toBuffer(self):
        return self.backend.download(self.ptr, self.rowCount * self.colCount * self.elementSize)

    def rowsToBuffers(self, indexes):
        """LowDegreeProver.ts:53,214,217 — one Buffer (colCount*elementSize bytes) per requested row."""
        return self.backend.gather(self.ptr, self.colCount * self.elementSize, list(indexes))

    def row(self, r):
        return Vector(self.backend, self.colCount, owner=self._owner, offset=self._offset + r * self.colCount * self.elementSize)


class PrimeField:
    """createPrimeField(modulus[, wasmOptions]) — index.ts:14; lib/Stark.ts:40."""

    def __init__(self, modulus=None, backend=None):
        """modulus None: the field the backend's library is built for (default library: the 128-bit field)."""
        self.backend = backend or Backend(modulus=modulus)
        if modulus is None:
            modulus = self.backend.modulus
        if modulus != self.backend.modulus:
            raise GstarkError(f'the backend computes in the field of {self.backend.modulus} elements, not {modulus}: '
                              'construct Backend(modulus=...) for one of the built fields')
        self._lastEvaluation = None     # (polys, ptr, omega, n, result) of the latest evalPolysAtRoots, weakly held
        self.modulus = modulus
        self.elementSize = self.backend.element_size   # 16 bytes; 32 in the 256- / 224-bit library flavours
        self.zero, self.one = 0, 1

    def le(self, v):
        return int(v).to_bytes(self.elementSize, 'little')

    # ---- scalar arithmetic (bigint in, bigint out)
    def mod(self, v): return v % self.modulus
    def add(self, a, b): return (a + b) % self.modulus
    def sub(self, a, b): return (a - b) % self.modulus
    def mul(self, a, b): return (a * b) % self.modulus
    def neg(self, a): return (-a) % self.modulus
    def inv(self, a): return pow(a, -1, self.modulus) if a % self.modulus else 0
    def div(self, a, b): return a * self.inv(b) % self.modulus

    def exp(self, base, exponent):
        if exponent < 0:  # examples/rescue/hash4x128.ts:14 passes a negative exponent
            return pow(self.inv(base), -exponent, self.modulus)
        return pow(base, exponent, self.modulus)

    def prng(self, seed, length=None):
        """FiniteField.prng (CompositionPolynomial.ts:58; LinearCombination.ts:58; LowDegreeProver.ts:194).
        Construction restated from galois' documented behaviour (UNVERIFIED)."""
        if length is None:
            return sha256_bigint(seed) % self.modulus
        out, state = [], sha256_bigint(seed)
        for _ in range(length):
            out.append(state % self.modulus)
            state = sha256_bigint(state)
        return self.newVectorFrom(out)

    def getRootOfUnity(self, order):
        """First i^((p-1)/order), i = 2,3,..., of exact order `order` (UNVERIFIED)."""
        if order <= 0 or order & (order - 1) or (self.modulus - 1) % order:
            raise GstarkError(f'Order {order} of root of unity is invalid')
        for i in range(2, 1 << 16):
            g = pow(i, (self.modulus - 1) // order, self.modulus)
            if pow(g, order, self.modulus) == 1 and (order == 1 or pow(g, order // 2, self.modulus) != 1):
                return g
        raise GstarkError(f'Root of unity for order {order} was not found')

    # ---- square roots (include/gstark_sqrt.h, csrc/sqrt.hip)
    MAX_SQRT_COUNT = 1 << 20

    def sqrt(self, a):
        """the even square root of a (as a canonical integer; the other one is p - root), or None for a non-residue"""
        return host_sqrt(int(a), self.modulus)

    @property
    def twoAdicity(self):
        """s of p - 1 = 2^s * t with t odd"""
        return host_two_adicity(self.modulus)

    def _sqrtEntries(self, who='PrimeField'):
        """whether the library takes roots on the device; a HIP library that lacks only these entries is an error: no quiet host path"""
        be = self.backend
        for name in ('gs_field_sqrt', 'gs_curve_lift_x', 'gs_curve_compress', 'gs_field_sqrt_plan'):
            if not hasattr(be.lib, name):
                if be.name == 'hip-gfx950':
                    raise GstarkError(f'{who}: the library has no {name} (include/gstark_sqrt.h)')
                return False
        return True

    def sqrtPlan(self):
        """gs_field_sqrt_plan: {'twoAdicity', 'windowBits', 'windows', 'productsPerRoot'} of the library's schedule, or None where it has none"""
        if not self._sqrtEntries():
            return None
        vals = [C.c_uint32() for _ in range(4)]
        self.backend.call('gs_field_sqrt_plan', *[C.byref(v) for v in vals])
        return dict(zip(('twoAdicity', 'windowBits', 'windows', 'productsPerRoot'), (v.value for v in vals)))

    def _sqrtOperand(self, v, what):
        if isinstance(v, Vector):
            if v.elementSize != self.elementSize:
                raise GstarkError(f'{what}: a vector of field elements, not of {v.elementSize}-byte entries')
            n, vec, vals = v.length, v, None
        else:
            try:
                vals = [int(x) for x in v]
            except (TypeError, ValueError):
                raise GstarkError(f'{what}: the values are integers') from None
            if any(not 0 <= x < self.modulus for x in vals):
                raise GstarkError(f'{what}: a value is not a canonical element')
            n, vec = len(vals), None
        if n > self.MAX_SQRT_COUNT:
            raise GstarkError(f'{what}: at most 2^20 elements per call, not {n}')
        return vec, vals, n

    def _flagVector(self, flags):
        out = Vector(self.backend, len(flags), element_size=1)
        if flags:
            self.backend.upload(out.ptr, bytes(flags))
        return out

    def sqrtVectorElements(self, v):
        """(roots, flags) of a Vector or a list of elements: a Vector of the even roots (0 where there is none) and a Vector of one-byte
        flags (1 = a square, 0 included); one launch, nothing read back"""
        vec, vals, n = self._sqrtOperand(v, 'sqrtVectorElements')
        if not self._sqrtEntries():
            roots = [host_sqrt(x, self.modulus) for x in (vals if vals is not None else vec.toValues())]
            return self.newVectorFrom([r or 0 for r in roots]), self._flagVector([r is not None for r in roots])
        roots, flags = Vector(self.backend, n), Vector(self.backend, n, element_size=1)
        if n:
            src = vec if vec is not None else self.newVectorFrom(vals)
            self.backend.call('gs_field_sqrt', C.c_void_p(src.ptr), n, C.c_void_p(roots.ptr), C.c_void_p(flags.ptr))
        return roots, flags

    def isSquareVectorElements(self, v):
        """the flags alone (Euler's criterion: one exponentiation, no table)"""
        vec, vals, n = self._sqrtOperand(v, 'isSquareVectorElements')
        if not self._sqrtEntries():
            p = self.modulus
            return self._flagVector([x == 0 or pow(x, (p - 1) // 2, p) == 1 for x in (vals if vals is not None else vec.toValues())])
        flags = Vector(self.backend, n, element_size=1)
        if n:
            src = vec if vec is not None else self.newVectorFrom(vals)
            self.backend.call('gs_field_sqrt', C.c_void_p(src.ptr), n, None, C.c_void_p(flags.ptr))
        return flags

    # ---- running sums, running products and linear recurrences (include/gstark_scan.h, csrc/scan.hip)
    MAX_SCAN_ELEMENTS = 1 << 24
    _SCAN_OPS = {'sum': 0, 'product': 1}

    def _scanEntries(self, who='PrimeField'):
        """whether the library scans on the device; a HIP library that lacks only these entries is an error: no quiet host path"""
        be = self.backend
        for name in ('gs_scan', 'gs_scan_affine', 'gs_reduce', 'gs_scan_plan'):
            if not hasattr(be.lib, name):
                if be.name == 'hip-gfx950':
                    raise GstarkError(f'{who}: the library has no {name} (include/gstark_scan.h)')
                return False
        return True

    def scanPlan(self, n=0):
        """gs_scan_plan: {'tile', 'elementsPerThread', 'maxElements', 'launches'} ('launches': what a call of n elements enqueues), or None
        where the library has none"""
        if not self._scanEntries():
            return None
        tile, per, most, launches = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
        self.backend.call('gs_scan_plan', int(n), C.byref(tile), C.byref(per), C.byref(most), C.byref(launches))
        return {'tile': tile.value, 'elementsPerThread': per.value, 'maxElements': most.value, 'launches': launches.value}

    def _scanCount(self, n, what):
        if n > self.MAX_SCAN_ELEMENTS:
            raise GstarkError(f'{what}: at most 2^24 elements per call, not {n}')
        return n

    def _scanValues(self, v, what):
        try:
            vals = [int(x) for x in v]
        except (TypeError, ValueError):
            raise GstarkError(f'{what}: the values are integers') from None
        if any(not 0 <= x < self.modulus for x in vals):
            raise GstarkError(f'{what}: a value is not a canonical element')
        return vals

    def _scanOperand(self, v, what):
        """(Vector or None, values or None, length) of a Vector or a list of canonical elements"""
        if isinstance(v, Vector):
            if v.elementSize != self.elementSize:
                raise GstarkError(f'{what}: a vector of field elements, not of {v.elementSize}-byte entries')
            return v, None, self._scanCount(v.length, what)
        if isinstance(v, Matrix):
            raise GstarkError(f'{what}: a Vector or a list, not a Matrix (the MatrixRows members take one)')
        self._scanCount(len(v) if hasattr(v, '__len__') else 0, what)
        vals = self._scanValues(v, what)
        return None, vals, len(vals)

    def _scanMatrix(self, m, what):
        """(Matrix or None, flat values or None, rows, cols) of a Matrix or a list of rows of equal length"""
        if isinstance(m, Matrix):
            if m.elementSize != self.elementSize:
                raise GstarkError(f'{what}: a matrix of field elements, not of {m.elementSize}-byte entries')
            rows, cols = m.rowCount, m.colCount
            if rows and not cols:
                raise GstarkError(f'{what}: {rows} rows of 0 columns')
            self._scanCount(rows * cols, what)
            return m, None, rows, cols
        if isinstance(m, Vector):
            raise GstarkError(f'{what}: a Matrix or a list of rows, not a Vector')
        rows = [list(r) for r in m]
        cols = len(rows[0]) if rows else 0
        if any(len(r) != cols for r in rows):
            raise GstarkError(f'{what}: the rows have different lengths')
        if rows and not cols:
            raise GstarkError(f'{what}: {len(rows)} rows of 0 columns')
        self._scanCount(len(rows) * cols, what)
        return None, self._scanValues([x for r in rows for x in r], what), len(rows), cols

    def _scanHeads(self, heads, n, what):
        """(Vector of bytes or None, list of flags or None): heads[i] & 1 starts a segment at i"""
        if heads is None:
            return None, None
        if isinstance(heads, Vector):
            if heads.elementSize != 1:
                raise GstarkError(f'{what}: heads is a vector of bytes, not of {heads.elementSize}-byte entries')
            if heads.length != n:
                raise GstarkError(f'{what}: {heads.length} heads and {n} values')
            return heads, None
        try:
            flags = [int(h) for h in heads]
        except (TypeError, ValueError):
            raise GstarkError(f'{what}: heads are bytes') from None
        if len(flags) != n:
            raise GstarkError(f'{what}: {len(flags)} heads and {n} values')
        if any(not 0 <= h < 256 for h in flags):
            raise GstarkError(f'{what}: heads are bytes')
        return None, flags

    @staticmethod
    def _hostFlags(n, cols, heads):
        """the head flag of every element: uniform segments of `cols`, or-ed with the low bit of the bytes"""
        return [i % cols == 0 or bool(heads is not None and heads[i] & 1) for i in range(n)]

    def _hostScan(self, op, vals, flags, exclusive):
        p, start = self.modulus, 0 if op == 'sum' else 1
        out, acc = [], start
        for v, h in zip(vals, flags):
            before = start if h else acc
            acc = (before + v) % p if op == 'sum' else before * v % p
            out.append(before if exclusive else acc)
        return out

    def _hostRecurrence(self, a, b, flags, x0, exclusive):
        p, out, x = self.modulus, [], x0
        for i, (bi, h) in enumerate(zip(b, flags)):
            before = x0 if h else x
            x = ((a if isinstance(a, int) else a[i]) * before + bi) % p
            out.append(before if exclusive else x)
        return out

    @staticmethod
    def _hostTotals(inclusive, rows, cols):
        return [inclusive[(r + 1) * cols - 1] for r in range(rows)]

    def _devicePtr(self, obj, vals):
        """the device object of an operand given as an object or as host values"""
        return obj if obj is not None else self.newVectorFrom(vals)

    def _scanVector(self, op, v, exclusive, heads, what):
        vec, vals, n = self._scanOperand(v, what)
        hvec, hlist = self._scanHeads(heads, n, what)
        if not self._scanEntries(what):
            vals = vals if vals is not None else vec.toValues()
            hlist = hlist if hvec is None else list(hvec.toBuffer())
            return self.newVectorFrom(self._hostScan(op, vals, self._hostFlags(n, max(n, 1), hlist), exclusive))
        out = Vector(self.backend, n)
        if n:
            src = self._devicePtr(vec, vals)
            if hlist is not None:
                hvec = self._flagVector(hlist)
            self.backend.call('gs_scan', self._SCAN_OPS[op], 1 if exclusive else 0, C.c_void_p(src.ptr), C.c_void_p(hvec.ptr) if hvec is not None else None, 1, n,
                              C.c_void_p(out.ptr), None)
        return out

    def prefixSumVectorElements(self, v, exclusive=False, heads=None):
        """the running sums of a Vector or a list, as a Vector: out[i] = v[0] + ... + v[i], or with exclusive=True v[0] + ... + v[i-1]
        (out[0] = 0).  heads (a Vector of bytes or a list, one per element): heads[i] & 1 starts a new segment at i, and segments
        never influence each other.  Nothing is read back."""
        return self._scanVector('sum', v, exclusive, heads, 'prefixSumVectorElements')

    def prefixProductVectorElements(self, v, exclusive=False, heads=None):
        """the running products: out[i] = v[0] * ... * v[i]; exclusive: out[0] = 1.  A zero zeroes the rest of its own segment only."""
        return self._scanVector('product', v, exclusive, heads, 'prefixProductVectorElements')

    def _scanRows(self, op, m, exclusive, totals, what):
        mat, vals, rows, cols = self._scanMatrix(m, what)
        n = rows * cols
        if not self._scanEntries(what):
            vals = vals if vals is not None else [x for r in mat.toValues() for x in r]
            flags = self._hostFlags(n, max(cols, 1), None)
            res = self._hostScan(op, vals, flags, exclusive)
            out = self.newMatrixFrom([res[r * cols:(r + 1) * cols] for r in range(rows)]) if n else Matrix(self.backend, rows, cols)
            if not totals:
                return out
            return out, self.newVectorFrom(self._hostTotals(res if not exclusive else self._hostScan(op, vals, flags, False), rows, cols))
        out, tot = Matrix(self.backend, rows, cols), Vector(self.backend, rows) if totals else None
        if n:
            src = mat if mat is not None else self.newVectorFrom(vals)
            self.backend.call('gs_scan', self._SCAN_OPS[op], 1 if exclusive else 0, C.c_void_p(src.ptr), None, rows, cols, C.c_void_p(out.ptr),
                              C.c_void_p(tot.ptr) if totals else None)
        return (out, tot) if totals else out

    def prefixSumMatrixRows(self, m, exclusive=False, totals=False):
        """the running sums of every row of a Matrix (or a list of rows) on its own, as a Matrix; with totals=True: (matrix, Vector of
        the rows' sums).  One call for all the rows."""
        return self._scanRows('sum', m, exclusive, totals, 'prefixSumMatrixRows')

    def prefixProductMatrixRows(self, m, exclusive=False, totals=False):
        """the running products of every row on its own; with totals=True: (matrix, Vector of the rows' products)"""
        return self._scanRows('product', m, exclusive, totals, 'prefixProductMatrixRows')

    def _reduceRows(self, op, src, vals, rows, cols, what):
        """a Vector of the `rows` totals of rows * cols elements given as a device object or as values"""
        n = rows * cols
        if not self._scanEntries(what):
            vals = vals if vals is not None else (src.toValues() if isinstance(src, Vector) else [x for r in src.toValues() for x in r])
            return self.newVectorFrom(self._hostTotals(self._hostScan(op, vals, self._hostFlags(n, max(cols, 1), None), False), rows, cols) if n else [])
        tot = Vector(self.backend, rows)
        if n:
            src = self._devicePtr(src, vals)
            self.backend.call('gs_reduce', self._SCAN_OPS[op], C.c_void_p(src.ptr), rows, cols, C.c_void_p(tot.ptr))
        return tot

    def _reduceVector(self, op, v, what):
        vec, vals, n = self._scanOperand(v, what)
        if not n:
            return 0 if op == 'sum' else 1
        return self._reduceRows(op, vec, vals, 1, n, what).getValue(0)

    def sumVectorElements(self, v):
        """the sum of a Vector or a list, as an integer: one element is read back"""
        return self._reduceVector('sum', v, 'sumVectorElements')

    def prodVectorElements(self, v):
        """the product of a Vector or a list, as an integer: one element is read back"""
        return self._reduceVector('product', v, 'prodVectorElements')

    def sumMatrixRows(self, m):
        """a Vector of the sums of the rows of a Matrix (or a list of rows); no running values are written"""
        mat, vals, rows, cols = self._scanMatrix(m, 'sumMatrixRows')
        return self._reduceRows('sum', mat, vals, rows, cols, 'sumMatrixRows')

    def prodMatrixRows(self, m):
        """a Vector of the products of the rows"""
        mat, vals, rows, cols = self._scanMatrix(m, 'prodMatrixRows')
        return self._reduceRows('product', mat, vals, rows, cols, 'prodMatrixRows')

    def _scanScalar(self, x, name, what):
        if isinstance(x, bool) or not isinstance(x, int):
            raise GstarkError(f'{what}: {name} is an integer')
        if not 0 <= x < self.modulus:
            raise GstarkError(f'{what}: {name} is not a canonical element')
        return x

    def _recurrence(self, a_obj, a_vals, a_scalar, b_obj, b_vals, rows, cols, heads, x0, exclusive, what):
        n = rows * cols
        hvec, hlist = heads
        if not self._scanEntries(what):
            flat = lambda o: o.toValues() if isinstance(o, Vector) else [x for r in o.toValues() for x in r]
            a = a_scalar if a_scalar is not None else (a_vals if a_vals is not None else flat(a_obj))
            b = b_vals if b_vals is not None else flat(b_obj)
            hlist = hlist if hvec is None else list(hvec.toBuffer())
            return self._hostRecurrence(a, b, self._hostFlags(n, max(cols, 1), hlist), x0, exclusive)
        out = _DeviceBuffer(self.backend, n * self.elementSize)
        if n:
            b_src = self._devicePtr(b_obj, b_vals)
            a_src = None if a_scalar is not None else self._devicePtr(a_obj, a_vals)
            if hlist is not None:
                hvec = self._flagVector(hlist)
            self.backend.call('gs_scan_affine', 1 if exclusive else 0, C.c_void_p(a_src.ptr) if a_src is not None else None, self.le(a_scalar) if a_scalar is not None else None,
                              C.c_void_p(b_src.ptr), self.le(x0), C.c_void_p(hvec.ptr) if hvec is not None else None, rows, cols, C.c_void_p(out.ptr))
        return out

    def linearRecurrence(self, a, b, x0=0, exclusive=False, heads=None):
        """x[i] = a[i] * x[i-1] + b[i] with x[-1] = x0, as a Vector: out[i] = x[i], or with exclusive=True x[i-1] (out[0] = x0).  a: a Vector,
        a list, or ONE integer for every step (a Horner chain, a geometric sum); b: a Vector or a list.  heads as in
        prefixSumVectorElements; x0 is ONE integer that starts every segment: a start that differs from segment to segment is folded
        into that segment's first b (b[first] + a[first] * start, x0 = 0).  Nothing is read back."""
        what = 'linearRecurrence'
        b_vec, b_vals, n = self._scanOperand(b, what)
        a_vec = a_vals = a_scalar = None
        if isinstance(a, int):
            a_scalar = self._scanScalar(a, 'a', what)
        else:
            a_vec, a_vals, na = self._scanOperand(a, what)
            if na != n:
                raise GstarkError(f'{what}: {na} factors and {n} terms: the lengths differ')
        x0 = self._scanScalar(x0, 'x0', what)
        res = self._recurrence(a_vec, a_vals, a_scalar, b_vec, b_vals, 1 if n else 0, n, self._scanHeads(heads, n, what), x0, exclusive, what)
        return self.newVectorFrom(res) if isinstance(res, list) else Vector(self.backend, n, owner=res)

    def linearRecurrenceMatrixRows(self, a, b, x0=0, exclusive=False):
        """linearRecurrence on every row of the matrices a and b (or lists of rows; a may be ONE integer) on its own, every row from x0"""
        what = 'linearRecurrenceMatrixRows'
        b_mat, b_vals, rows, cols = self._scanMatrix(b, what)
        a_mat = a_vals = a_scalar = None
        if isinstance(a, int):
            a_scalar = self._scanScalar(a, 'a', what)
        else:
            a_mat, a_vals, ra, ca = self._scanMatrix(a, what)
            if (ra, ca) != (rows, cols):
                raise GstarkError(f'{what}: a is {ra} x {ca} and b is {rows} x {cols}: the shapes differ')
        x0 = self._scanScalar(x0, 'x0', what)
        res = self._recurrence(a_mat, a_vals, a_scalar, b_mat, b_vals, rows, cols, (None, None), x0, exclusive, what)
        if isinstance(res, list):
            return self.newMatrixFrom([res[r * cols:(r + 1) * cols] for r in range(rows)]) if rows * cols else Matrix(self.backend, rows, cols)
        return Matrix(self.backend, rows, cols, owner=res)

    # ---- construction
    def newVector(self, length):
        return Vector(self.backend, length)

    def newVectorFrom(self, values):
        v = Vector(self.backend, len(values))
        if values:
            self.backend.upload(v.ptr, b''.join(self.le(x % self.modulus) for x in values))
        return v

    def newMatrix(self, rows, cols):
        return Matrix(self.backend, rows, cols)

    def newMatrixFrom(self, values):
        rows, cols = len(values), len(values[0]) if values else 0
        m = Matrix(self.backend, rows, cols)
        if rows * cols:
            self.backend.upload(m.ptr, b''.join(self.le(x % self.modulus) for r in values for x in r))
        return m

    def newMatrixFromVectors(self, vectors):
        # rows shorter than the longest one are zero-extended (polynomials of different degrees, e.g. boundary
        # interpolants of registers with different numbers of assertions: BoundaryConstraints.ts:84-85)
        cols = max(v.length for v in vectors)
        m = Matrix(self.backend, len(vectors), cols)
        for r, v in enumerate(vectors):
            self.backend.call('gs_copy', C.c_void_p(m.ptr + r * cols * self.elementSize), C.c_void_p(v.ptr), v.length * self.elementSize)
            if v.length < cols:
                self.backend.upload(m.ptr + (r * cols + v.length) * self.elementSize, bytes((cols - v.length) * self.elementSize))
        return m

    def matrixRowsToVectors(self, matrix):
        return [matrix.row(r) for r in range(matrix.rowCount)]

    # ---- vector operations
    def _binary(self, fn_vec, fn_scalar, a, b):
        out = Vector(self.backend, a.length)
        if isinstance(b, int):
            self.backend.call(fn_scalar, C.c_void_p(a.ptr), self.le(b % self.modulus), a.length, C.c_void_p(out.ptr))
        else:
            if a.length != b.length:
                raise GstarkError('Cannot combine vector elements: vectors have different lengths')
            self.backend.call(fn_vec, C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.length, C.c_void_p(out.ptr))
        return out

    def addVectorElements(self, a, b): return self._binary('gs_vec_add', 'gs_vec_add_scalar', a, b)
    def subVectorElements(self, a, b): return self._binary('gs_vec_sub', 'gs_vec_sub_scalar', a, b)
    def mulVectorElements(self, a, b): return self._binary('gs_vec_mul', 'gs_vec_mul_scalar', a, b)

    def divVectorElements(self, a, b):
        if isinstance(b, int):
            return self.mulVectorElements(a, self.inv(b))
        if a.length != b.length:
            raise GstarkError('Cannot divide vector elements: vectors have different lengths')
        out = Vector(self.backend, a.length)
        self.backend.call('gs_vec_div', C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.length, C.c_void_p(out.ptr))
        return out

    def invVectorElements(self, a):
        out = Vector(self.backend, a.length)
        self.backend.call('gs_vec_inv', C.c_void_p(a.ptr), a.length, C.c_void_p(out.ptr))
        return out

    def expVectorElements(self, a, e):
        out = Vector(self.backend, a.length)
        if e < 0:
            a, e = self.invVectorElements(a), -e
        self.backend.call('gs_vec_exp', C.c_void_p(a.ptr), self.le(e), a.length, C.c_void_p(out.ptr))
        return out

    # ---- fused forms of divisions whose denominators are known in closed form over the domain (no counterpart in galois: same
    # values as the member sequences named in include/gstark.h, one kernel each)
    fusedDomainDivisions = True          # the components ask before using the two members below (a distributed field says no)

    def zeroPolyInverses(self, rootOfUnity, domainSize, steps, xAtLastStep):
        """1/Z(x) over the evaluation domain: ZeroPolynomial.evaluateAll + CompositionPolynomial.ts:117 (den / num)."""
        out = Vector(self.backend, domainSize)
        self.backend.call('gs_zero_poly_inverses', self.le(rootOfUnity), domainSize, steps, self.le(xAtLastStep), C.c_void_p(out.ptr))
        return out

    MAX_DOMAIN_ROOTS = 4

    def divByDomainRoots(self, numerators, rootOfUnity, rootIndexes):
        """numerators[r][i] / prod_k (omega^i - omega^k), k in rootIndexes[r]: BoundaryConstraints.ts:87-92 when every divisor's
        roots are domain points (at most MAX_DOMAIN_ROOTS per row)."""
        rows, n = numerators.rowCount, numerators.colCount
        width = max(len(r) for r in rootIndexes)
        flat = (C.c_uint64 * (rows * width))(*[(r[a] if a < len(r) else 0) for r in rootIndexes for a in range(width)])
        counts = (C.c_uint32 * rows)(*[len(r) for r in rootIndexes])
        out = Matrix(self.backend, rows, n)
        self.backend.call('gs_div_by_domain_roots', C.c_void_p(numerators.ptr), rows, n, self.le(rootOfUnity), flat, counts, width, C.c_void_p(out.ptr))
        return out

    def combineVectors(self, a, b):
        if a.length != b.length:
            raise GstarkError('Cannot combine vectors: vectors have different lengths')
        buf = C.create_string_buffer(self.elementSize)
        self.backend.call('gs_combine', C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.length, C.cast(buf, C.c_void_p))
        return int.from_bytes(buf.raw, 'little')

    def combineManyVectors(self, vectors, coefficients):
        ks = coefficients.toValues() if isinstance(coefficients, Vector) else list(coefficients)
        if len(ks) != len(vectors):
            raise GstarkError('Number of coefficients must be the same as the number of vectors')
        n = vectors[0].length
        out = Vector(self.backend, n)
        self.backend.call('gs_combine_many', Backend.ptr_array([v.ptr for v in vectors]),
                          b''.join(self.le(k) for k in ks), len(vectors), n, C.c_void_p(out.ptr))
        return out

    def getPowerSeries(self, base, length):
        out = Vector(self.backend, length)
        self.backend.call('gs_power_series', self.le(base), length, C.c_void_p(out.ptr))
        out.series_base = base % self.modulus
        return out

    def pluckVector(self, v, skip, times):
        out = Vector(self.backend, times)
        self.backend.call('gs_pluck', C.c_void_p(v.ptr), v.length, skip, times, C.c_void_p(out.ptr))
        return out

    def transposeVector(self, v, columns, step=1):
        if v.length % (columns * step):
            raise GstarkError('Number of columns must evenly divide vector length')
        rows = v.length // (columns * step)
        m = Matrix(self.backend, rows, columns)
        self.backend.call('gs_transpose_vector', C.c_void_p(v.ptr), v.length, columns, step, C.c_void_p(m.ptr))
        if columns == 4 and v.series_base is not None:
            m.quartic_domain = (v.series_base, v.length, step)
        return m

    # ---- matrix operations
    def transposeMatrix(self, m):
        out = Matrix(self.backend, m.colCount, m.rowCount)
        self.backend.call('gs_transpose_matrix', C.c_void_p(m.ptr), m.rowCount, m.colCount, C.c_void_p(out.ptr))
        return out

    def mulMatrixByVector(self, m, v):
        """galois FiniteField.mulMatrixByVector (examples/poseidon/utils.ts:45: `mds x state`): out[r] = sum_c m[r][c] * v[c],
        one device dot product per row."""
        if m.colCount != v.length:
            raise GstarkError('Matrix column count must be the same as vector length')
        return self.newVectorFrom([self.combineVectors(m.row(r), v) for r in range(m.rowCount)])

    def joinMatrixRows(self, m):
        return Vector(self.backend, m.rowCount * m.colCount, owner=m._owner, offset=m._offset)

    def subMatrixElementsFromVectors(self, vectors, m):
        out = Matrix(self.backend, m.rowCount, m.colCount)
        self.backend.call('gs_sub_matrix_from_vectors', Backend.ptr_array([v.ptr for v in vectors]),
                          C.c_void_p(m.ptr), m.rowCount, m.colCount, C.c_void_p(out.ptr))
        return out

    def divMatrixElements(self, a, b):
        out = Matrix(self.backend, a.rowCount, a.colCount)
        self.backend.call('gs_vec_div', C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.rowCount * a.colCount, C.c_void_p(out.ptr))
        return out

    # ---- polynomials
    def _omega_of(self, roots):
        if roots.series_base is not None:
            return roots.series_base
        return roots.getValue(1) if roots.length > 1 else 1

    def evalPolyAtRoots(self, poly, roots):
        """CompositionPolynomial.ts:110 — NTT of `poly` (zero-extended) over the roots-of-unity vector."""
        if poly.length > roots.length:
            raise GstarkError('Number of roots of unity cannot be smaller than number of values')
        out = Vector(self.backend, roots.length)
        self.backend.call('gs_eval_polys_at_roots', C.c_void_p(poly.ptr), 1, poly.length, self.le(self._omega_of(roots)),
                          roots.length, C.c_void_p(out.ptr))
        return out

    def evalPolysAtRoots(self, polys, roots):
        """lib/Stark.ts:109; BoundaryConstraints.ts:87-88.  The evaluations of the SAME polynomials over a subgroup of the
        domain they were last evaluated on (the composition domain after the evaluation domain: lib/Stark.ts:109 then
        CompositionPolynomial.ts:76) are every k-th element of that result: a strided copy instead of another NTT."""
        if polys.colCount > roots.length:
            raise GstarkError('Number of roots of unity cannot be smaller than number of values')
        n, omega = roots.length, self._omega_of(roots)
        out = Matrix(self.backend, polys.rowCount, n)
        prev = self._lastEvaluation
        if prev is not None:
            ppolys, pptr, pomega, pn, pout = prev[0](), prev[1], prev[2], prev[3], prev[4]()
            if ppolys is polys and pptr == polys.ptr and pout is not None and pn > n and pn % n == 0 and \
                    pow(pomega, pn // n, self.modulus) == omega:
                for r in range(polys.rowCount):
                    self.backend.call('gs_pluck', C.c_void_p(pout.ptr + r * pn * self.elementSize), pn, pn // n, n,
                                      C.c_void_p(out.ptr + r * n * self.elementSize))
                return out
        self.backend.call('gs_eval_polys_at_roots', C.c_void_p(polys.ptr), polys.rowCount, polys.colCount, self.le(omega), n,
                          C.c_void_p(out.ptr))
        self._lastEvaluation = (weakref.ref(polys), polys.ptr, omega, n, weakref.ref(out))
        return out

    def interpolateRoots(self, roots, ys):
        """lib/Stark.ts:106; CompositionPolynomial.ts:109 — inverse NTT (Vector or Matrix of rows)."""
        n = roots.length
        if isinstance(ys, Matrix):
            if ys.colCount != n:
                raise GstarkError('Number of roots of unity must be the same as the number of y coordinates')
            out = Matrix(self.backend, ys.rowCount, n)
            rows = ys.rowCount
        else:
            if ys.length != n:
                raise GstarkError('Number of roots of unity must be the same as the number of y coordinates')
            out, rows = Vector(self.backend, n), 1
        self.backend.call('gs_interpolate_roots', C.c_void_p(ys.ptr), rows, self.le(self._omega_of(roots)), n, C.c_void_p(out.ptr))
        return out

    def evalPolyAt(self, poly, x):
        buf = C.create_string_buffer(self.elementSize)
        self.backend.call('gs_eval_poly_at', C.c_void_p(poly.ptr), poly.length, self.le(x), C.cast(buf, C.c_void_p))
        return int.from_bytes(buf.raw, 'little')

    def evalPolysAtPoints(self, polys, xs):
        """The rows of `polys` (a Matrix of coefficients, or a list of Vectors) at every x of `xs` (integers; any points, not roots of a
        transform): a Matrix, [r][k] = p_r(xs[k]).  One launch and no read-back where the library has gs_eval_polys_at_points
        (include/gstark_boundary.h); one evalPolyAt per polynomial and point on a library without it."""
        xs = [x % self.modulus for x in xs]
        rows = [polys.row(r) for r in range(polys.rowCount)] if isinstance(polys, Matrix) else list(polys)
        out = Matrix(self.backend, len(rows), len(xs))
        if not rows or not xs:
            return out
        if not hasattr(self.backend.lib, 'gs_eval_polys_at_points'):
            values = b''.join(self.le(self.evalPolyAt(p, x)) for p in rows for x in xs)
            self.backend.upload(out.ptr, values)
            return out
        if isinstance(polys, Matrix):
            src, stride, lens = polys, polys.colCount, [polys.colCount] * len(rows)
        else:       # vectors of any lengths, side by side in rows of the longest
            stride, lens = max(p.length for p in rows), [p.length for p in rows]
            src = Matrix(self.backend, len(rows), max(stride, 1))
            for r, p in enumerate(rows):
                if p.length:
                    self.backend.call('gs_copy', C.c_void_p(src.ptr + r * stride * self.elementSize), C.c_void_p(p.ptr), p.length * self.elementSize)
        self.backend.call('gs_eval_polys_at_points', C.c_void_p(src.ptr), len(rows), stride, (C.c_uint64 * len(rows))(*lens),
                          b''.join(self.le(x) for x in xs), len(xs), C.c_void_p(out.ptr))
        return out

    def mulPolys(self, a, b):
        """BoundaryConstraints.ts:30 — product of two polynomials.  The reference only multiplies tiny ones (degree <= number
        of assertions): those stay on the host; larger operands go through the device NTT (evaluate both on a domain of
        >= len(a)+len(b)-1 roots, multiply pointwise, interpolate)."""
        la, lb = a.length, b.length
        if la * lb <= 4096:
            av, bv = a.toValues(), b.toValues()
            out = [0] * (la + lb - 1)
            for i, x in enumerate(av):
                for j, y in enumerate(bv):
                    out[i + j] = (out[i + j] + x * y) % self.modulus
            return self.newVectorFrom(out)
        n = 1 << (la + lb - 2).bit_length()
        roots = self.getPowerSeries(self.getRootOfUnity(n), n)
        prod = self.mulVectorElements(self.evalPolyAtRoots(a, roots), self.evalPolyAtRoots(b, roots))
        full = self.interpolateRoots(roots, prod)
        return Vector(self.backend, la + lb - 1, owner=full._owner, offset=full._offset)

    def _pad_poly(self, v, length):
        if v.length == length:
            return v
        out = Vector(self.backend, length)
        self.backend.call('gs_copy', C.c_void_p(out.ptr), C.c_void_p(v.ptr), v.length * self.elementSize)
        self.backend.upload(out.ptr + v.length * self.elementSize, bytes((length - v.length) * self.elementSize))
        return out

    def addPolys(self, a, b):
        """galois FiniteField.addPolys: coefficient-wise sum, the shorter operand zero-extended."""
        n = max(a.length, b.length)
        return self.addVectorElements(self._pad_poly(a, n), self._pad_poly(b, n))

    def subPolys(self, a, b):
        n = max(a.length, b.length)
        return self.subVectorElements(self._pad_poly(a, n), self._pad_poly(b, n))

    def mulPolyByConstant(self, a, c):
        return self.mulVectorElements(a, c % self.modulus)

    # ---- long polynomials at arbitrary points (include/gstark_poly.h, csrc/poly.hip): n log^2 n field products where
    # `interpolate` and `evalPolysAtPoints` (both unchanged) take n^2.  Operands are Vectors or lists, results stay on the device.  On a
    # library without the entries (the tests' double) the same values come from host integers by the quadratic definitions
    MAX_POLY_LENGTH = 1 << 20
    # evalPolyAtPoints(method=None) leaves Horner for the tree when coefficients and points both reach this many; None: never.  From
    # profiles/poly.md (len = points, 128-bit | 224-bit flavour): Horner ahead at 2^14 (0.69 against 2.12 ms | 3.21 against 9.10), the
    # tree at 2^15 (2.48 against 2.61 | 10.4 against 12.5) and by 3.4 x | 4.1 x at 2^16; other shapes were not measured
    TREE_EVAL_FROM = 1 << 15

    def _polyEntries(self):
        """whether the library computes these on the device; a HIP library that lacks only these entries is an error: no quiet host path"""
        be = self.backend
        for name in ('gs_poly_from_roots', 'gs_poly_div', 'gs_poly_eval_points', 'gs_poly_interpolate_points'):
            if not hasattr(be.lib, name):
                if be.name == 'hip-gfx950':
                    raise GstarkError(f'PrimeField: the library has no {name} (include/gstark_poly.h)')
                return False
        return True

    def _polyOmega(self):
        """(omega, log2 of its order): getRootOfUnity of the largest power of two that divides p - 1, capped at 2^26; once per field object"""
        if getattr(self, '_poly_omega', None) is None:
            log2 = min(((self.modulus - 1) & -(self.modulus - 1)).bit_length() - 1, 26)
            self._poly_omega = (self.le(self.getRootOfUnity(1 << log2)), log2)
        return self._poly_omega

    def _polyOperand(self, v, what):
        """(a device Vector | None, host values | None, length) of a Vector or a list of integers"""
        if isinstance(v, Vector):
            n, vec, vals = v.length, v, None
        else:
            vals = [int(x) % self.modulus for x in v]
            n, vec = len(vals), None
        if n > self.MAX_POLY_LENGTH:
            raise GstarkError(f'{what}: at most 2^20 elements per operand, not {n}')
        return vec, vals, n

    def _polyDevice(self, vec, vals):
        return vec if vec is not None else self.newVectorFrom(vals)

    @staticmethod
    def _polyHost(vec, vals):
        return vals if vals is not None else vec.toValues()

    def polyFromRoots(self, xs):
        """the len(xs) + 1 coefficients of prod (x - xs[i]), low-order first; no root: the polynomial 1"""
        vec, vals, n = self._polyOperand(xs, 'polyFromRoots')
        if not self._polyEntries():
            out = [1]
            for x in self._polyHost(vec, vals):
                out = _host_mul_linear(out, x, self.modulus)
            return self.newVectorFrom(out)
        omega, log2 = self._polyOmega()
        out = Vector(self.backend, n + 1)
        src = self._polyDevice(vec, vals) if n else None
        self.backend.call('gs_poly_from_roots', omega, log2, C.c_void_p(src.ptr) if n else None, n, C.c_void_p(out.ptr))
        return out

    def divModPolys(self, a, b):
        """(q, r) with a = q * b + r: q has len(a) - len(b) + 1 coefficients (one zero when a is shorter than b), r has len(b) - 1 (high
        zeros included).  The last coefficient of b must not be zero."""
        avec, avals, la = self._polyOperand(a, 'divModPolys')
        bvec, bvals, lb = self._polyOperand(b, 'divModPolys')
        if not la or not lb:
            raise GstarkError('divModPolys: both polynomials need at least one coefficient')
        if not self._polyEntries():
            av, bv = self._polyHost(avec, avals), self._polyHost(bvec, bvals)
            if not bv[-1]:
                raise GstarkError('divModPolys: the leading coefficient of b is zero')
            q, r = _host_divmod(av, bv, self.modulus)
            return self.newVectorFrom(q), self.newVectorFrom(r)
        omega, log2 = self._polyOmega()
        q, r = Vector(self.backend, max(la - lb + 1, 1)), Vector(self.backend, lb - 1)
        asrc, bsrc = self._polyDevice(avec, avals), self._polyDevice(bvec, bvals)      # (held until the call is enqueued)
        self.backend.call('gs_poly_div', omega, log2, C.c_void_p(asrc.ptr), la, C.c_void_p(bsrc.ptr), lb, C.c_void_p(q.ptr), C.c_void_p(r.ptr))
        return q, r

    def divPolys(self, a, b):
        """galois FiniteField.divPolys: the quotient of divModPolys"""
        return self.divModPolys(a, b)[0]

    def evalPolyAtPoints(self, poly, xs, method=None):
        """poly at every x of xs (any points; repeats allowed): a Vector.  method 'horner': gs_eval_polys_at_points, len(poly) * len(xs)
        products; 'tree': down the subproduct tree of the points (gs_poly_eval_points); None: whichever profiles/poly.md found faster
        at this size (TREE_EVAL_FROM)."""
        if method not in (None, 'tree', 'horner'):
            raise GstarkError(f"evalPolyAtPoints: method {method!r} is not 'tree', 'horner' or None")
        pvec, pvals, plen = self._polyOperand(poly, 'evalPolyAtPoints')
        xvec, xvals, n = self._polyOperand(xs, 'evalPolyAtPoints')
        if method is None:
            method = 'tree' if self.TREE_EVAL_FROM is not None and min(plen, n) >= self.TREE_EVAL_FROM else 'horner'
        if method == 'horner':
            if not n or not plen:
                return self.newVectorFrom([0] * n)
            return self.evalPolysAtPoints([self._polyDevice(pvec, pvals)], self._polyHost(xvec, xvals)).row(0)
        if not self._polyEntries():
            return self.newVectorFrom(_host_eval(self._polyHost(pvec, pvals), self._polyHost(xvec, xvals), self.modulus))
        omega, log2 = self._polyOmega()
        out = Vector(self.backend, n)
        psrc, xsrc = self._polyDevice(pvec, pvals), self._polyDevice(xvec, xvals)
        self.backend.call('gs_poly_eval_points', omega, log2, C.c_void_p(psrc.ptr) if plen else None, plen, C.c_void_p(xsrc.ptr) if n else None, n,
                          C.c_void_p(out.ptr) if n else None)
        return out

    def interpolateAtPoints(self, xs, ys):
        """the len(xs) coefficients of the polynomial through (xs[i], ys[i]): any distinct points, any number up to 2^20 (`interpolate`
        keeps its host route and its cap).  Two equal xs raise."""
        xvec, xvals, n = self._polyOperand(xs, 'interpolateAtPoints')
        yvec, yvals, ny = self._polyOperand(ys, 'interpolateAtPoints')
        if n != ny:
            raise GstarkError('Number of x coordinates must be the same as number of y coordinates')
        if not n:
            raise GstarkError('interpolateAtPoints: at least one point')
        if not self._polyEntries():
            xv, yv = self._polyHost(xvec, xvals), self._polyHost(yvec, yvals)
            if len(set(xv)) != n:
                raise GstarkError('interpolateAtPoints: two of the x coordinates are equal')
            return self.newVectorFrom(_host_interpolate(xv, yv, self.modulus))
        omega, log2 = self._polyOmega()
        out, flag = Vector(self.backend, n), Vector(self.backend, 1, element_size=1)
        xsrc, ysrc = self._polyDevice(xvec, xvals), self._polyDevice(yvec, yvals)
        self.backend.call('gs_poly_interpolate_points', omega, log2, C.c_void_p(xsrc.ptr), C.c_void_p(ysrc.ptr), n, C.c_void_p(out.ptr), C.c_void_p(flag.ptr))
        if self.backend.download(flag.ptr, 1)[0]:
            raise GstarkError('interpolateAtPoints: two of the x coordinates are equal')
        return out

    def interpolate(self, xs, ys):
        """BoundaryConstraints.ts:42; LowDegreeProver.ts:243 — Lagrange through a handful of points: O(n^2) host
        arithmetic inside the library (gs_small_interpolate), as in the reference's JS layer."""
        # xs known to be a whole domain {g^i} of a power-of-two order (getPowerSeries of a root of unity) and a library with the device
        # entry point: the same coefficients without the host path's 4 096-point cap
        base, n = getattr(xs, 'series_base', None), getattr(xs, 'length', 0)
        if base is not None and n > 1 and not n & (n - 1) and n == (len(ys) if isinstance(ys, (list, tuple)) else ys.length) \
                and hasattr(self.backend.lib, 'gs_boundary_polys') and pow(base, n // 2, self.modulus) == self.modulus - 1 \
                and (self.modulus - 1) % (2 * n) == 0:
            return self.interpolateAtRoots(base, n, list(range(n)), ys)
        xv = xs if isinstance(xs, (list, tuple)) else xs.toValues()
        yv = ys if isinstance(ys, (list, tuple)) else ys.toValues()
        if len(xv) != len(yv):
            raise GstarkError('Number of x coordinates must be the same as number of y coordinates')
        return self.newVectorFrom(self.interpolateValues(xv, yv))

    def _rootAbove(self, g, order):
        """a square root of g (g of order `order`, a power of two): an element of order 2 * order, found in the field's 2-power subgroup bit by bit"""
        p = self.modulus
        w = self.getRootOfUnity(2 * order)
        g0, e = w * w % p, 0
        for i in range(order.bit_length() - 1):
            if pow(g * pow(pow(g0, e, p), p - 2, p) % p, order >> (i + 1), p) != 1:
                e |= 1 << i
        s = pow(w, e, p)
        if s * s % p != g % p:
            raise GstarkError(f'interpolateAtRoots: {g} does not generate a domain of {order} points')
        return s

    def interpolateAtRoots(self, rootOfUnity, order, positions, ys):
        """The interpolant through (rootOfUnity^positions[i], ys[i]): points of the domain of `order` points (a power of two) that rootOfUnity
        generates — any generator of it —, distinct positions; built on the device (gs_boundary_polys): any number of points up
        to `order`, a device vector of len(positions) coefficients, the ones `interpolate` gives for these points.  The field must have a
        root of unity of order 2 * order (so not its largest power-of-two domain), the library the entry point (the HIP library has it);
        `interpolate` remains for everything else (host, at most 4 096 points)."""
        yv = ys if isinstance(ys, (list, tuple)) else ys.toValues()
        m = len(positions)
        if m != len(yv):
            raise GstarkError('Number of x coordinates must be the same as number of y coordinates')
        if m < 1 or order < 1 or order & (order - 1):
            raise GstarkError('interpolateAtRoots: at least one point, on a domain of a power-of-two order')
        if not hasattr(self.backend.lib, 'gs_boundary_polys'):
            raise GstarkError('this library has no gs_boundary_polys: use interpolate')
        omega = self._rootAbove(rootOfUnity % self.modulus, order)
        out, z = Vector(self.backend, m), Vector(self.backend, m + 1)
        self.backend.call('gs_boundary_polys', self.le(omega), 2 * order, order, (C.c_uint64 * m)(*positions),
                          b''.join(self.le(y % self.modulus) for y in yv), (C.c_uint32 * 1)(m), 1, m, C.c_void_p(out.ptr), C.c_void_p(z.ptr))
        return out

    def interpolateValues(self, xv, yv):
        n = len(xv)
        es = self.elementSize
        out = C.create_string_buffer(es * n)
        rc = self.backend.lib.gs_small_interpolate(b''.join(self.le(x % self.modulus) for x in xv),
                                                   b''.join(self.le(y % self.modulus) for y in yv), n, C.cast(out, C.c_void_p))
        if rc:
            raise GstarkError(f'gs_small_interpolate failed ({rc})')
        raw = out.raw
        return [int.from_bytes(raw[es * i:es * i + es], 'little') for i in range(n)]

    def evalPolyAtMany(self, poly_values, xs):
        """evalPolyAt over a list of points (LowDegreeProver.ts:246-251), host arithmetic inside the library."""
        m = len(xs)
        es = self.elementSize
        out = C.create_string_buffer(es * max(m, 1))
        rc = self.backend.lib.gs_small_eval_poly(b''.join(self.le(c) for c in poly_values), len(poly_values),
                                                 b''.join(self.le(x) for x in xs), m, C.cast(out, C.c_void_p))
        if rc:
            raise GstarkError(f'gs_small_eval_poly failed ({rc})')
        raw = out.raw
        return [int.from_bytes(raw[es * i:es * i + es], 'little') for i in range(m)]

    def interpolateQuarticBatch(self, xs, ys):
        """LowDegreeProver.ts:137,191 — one cubic per row.  When xs is the transposed power-series domain
        the prover builds (LowDegreeProver.ts:190) the x coordinates are regenerated on the fly."""
        if xs.rowCount != ys.rowCount or xs.colCount != 4 or ys.colCount != 4:
            raise GstarkError('X and Y coordinate matrixes must have the same shape with 4 columns')
        out = Matrix(self.backend, ys.rowCount, 4)
        if xs.quartic_domain is not None:
            omega, n, step = xs.quartic_domain
            self.backend.call('gs_interpolate_quartic_domain', self.le(omega), n, step, C.c_void_p(ys.ptr), ys.rowCount,
                              C.c_void_p(out.ptr))
        else:
            self.backend.call('gs_interpolate_quartic_batch', C.c_void_p(xs.ptr), C.c_void_p(ys.ptr), ys.rowCount,
                              C.c_void_p(out.ptr))
        return out

    def evalQuarticBatch(self, polys, x):
        out = Vector(self.backend, polys.rowCount)
        self.backend.call('gs_eval_quartic_batch', C.c_void_p(polys.ptr), polys.rowCount, self.le(x), C.c_void_p(out.ptr))
        return out


def createPrimeField(modulus=MODULUS, backend=None):
    return PrimeField(modulus, backend)
