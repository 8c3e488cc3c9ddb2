"""Scalar multiplications on short Weierstrass curves y^2 = x^3 + a*x + b over a field, in batches on the device
(include/gstark_curve.h, csrc/curve.hip): the numbers the reference's elliptic-curve statements assert — the product k*P of
examples/elliptic/pointmul.aa, and the public key x*G, the nonce point k*G and the check s*G = R + h*P of VerifySchnorrSignature
(assembly/lib224.aa) — which `pointmul.ec_multiply` (the control) computes one point at a time on Python integers.

A point is a pair (x, y) of integers, the point at infinity is None.  `Curve.mulMany` is ONE launch for the whole batch: one thread per
multiplication.  On a backend whose library lacks the entry points (the tests' double) the same values come from host integers through
one complete affine addition (`Curve.add`).

`Curve.msm` is the SUM of such products, sum_k scalars[k] * points[k], in one call that reads nothing back (include/gstark_msm.h,
csrc/msm.hip: the bucket method), `Curve.sumMany` the sum of the points themselves, and `schnorr_verify_batch` the one equation that
checks a whole block of signatures with one such sum."""
import ctypes as C
import secrets as _secrets

from ._abi import MODULUS_224, GstarkError
from .field import Matrix, Vector, host_sqrt

MAX_COUNT = 1 << 20          # multiplications per call (gs_curve_mul), terms per sum (gs_curve_msm)
MAX_WINDOW = 16              # the widest window gs_curve_msm can be forced to
MAX_BATCH = (1 << 19) - 1    # signatures per schnorr_verify_batch: 2 * count + 1 terms of one sum
SCALAR_BITS = 256

# the curve of pointmul.aa / lib224.aa with the point the reference's examples multiply (pointMul.ts:23-24, lib224.ts:163: the generator
# of NIST P-224); b follows from the point (Gy^2 - Gx^3 - a*Gx), and ORDER_224 * G is infinity
G_224 = (19277929113566293071110308034699488026831934219452440156649784352033, 19926808758034470970197974370888749184205991990603949537637343198772)
B_224 = 0xb4050a850c04b3abf54132565044b0b7d7bfd8ba270b39432355ffb4
ORDER_224 = 0xffffffffffffffffffffffffffff16a2e0b8f03e13dd29455c5c2a3d


class Curve:
    """y^2 = x^3 + a*x + b over `field` (a PrimeField, or a HostField: host integers only).  `G` and `order` are None unless the maker
    of the curve knows a base point (curve224)."""

    def __init__(self, field, a, b, G=None, order=None):
        p = field.modulus
        self.field, self.a, self.b = field, int(a) % p, int(b) % p
        self.G, self.order = G, order
        if G is not None and not self.contains(G):
            raise GstarkError('Curve: the base point is not on the curve')

    # ---- host integers
    def contains(self, point):
        if point is None:
            return True
        p = self.field.modulus
        x, y = point
        return 0 <= x < p and 0 <= y < p and (y * y - (x * x + self.a) * x - self.b) % p == 0

    def neg(self, point):
        return None if point is None else (point[0], -point[1] % self.field.modulus)

    def add(self, u, v):
        """the affine group law, complete: infinity, equal points, opposite points, points with y = 0"""
        if u is None: return v
        if v is None: return u
        p = self.field.modulus
        if u[0] == v[0]:
            if (u[1] + v[1]) % p == 0:
                return None                                            # opposite points; a point with y = 0 is its own opposite
            m = (3 * u[0] * u[0] + self.a) * pow(2 * u[1], -1, p) % p
        else:
            m = (u[1] - v[1]) * pow(u[0] - v[0], -1, p) % p
        x = (m * m - u[0] - v[0]) % p
        return x, (m * (u[0] - x) - u[1]) % p

    def _hostMul(self, point, scalar):
        acc = None
        for i in reversed(range(scalar.bit_length())):
            acc = self.add(acc, acc)
            if (scalar >> i) & 1:
                acc = self.add(acc, point)
        return acc

    # ---- device
    def _has(self, names, header):
        be = getattr(self.field, 'backend', None)
        if be is None:
            return False
        for name in names:
            if not hasattr(be.lib, name):
                if be.name == 'hip-gfx950':
                    raise GstarkError(f'Curve: the library has no {name} ({header})')
                return False
        return True

    @property
    def onDevice(self):
        """False on a library without the entry points (the tests' double) and on a HostField: host integers.  A device library that
        lacks only these entries is an error: no quiet host path."""
        return self._has(('gs_curve_mul', 'gs_curve_contains'), 'include/gstark_curve.h')

    @property
    def sumsOnDevice(self):
        """the same for `msm` and `sumMany` (gs_curve_msm); `mulMany` does not need it"""
        return self._has(('gs_curve_msm',), 'include/gstark_msm.h')

    def _readPoints(self, points, what, count=None):
        """(a device Matrix of rows x 2 | a list of (x, y)), rows"""
        if isinstance(points, Matrix):
            if points.colCount != 2:
                raise GstarkError(f'Curve: a matrix of {what} has 2 columns (x, y), not {points.colCount}')
            return points, points.rowCount
        points = list(points)
        if count is None and len(points) == 2 and all(isinstance(v, int) for v in points):
            points = [points]                                          # one (x, y) for all
        try:
            points = [(int(x), int(y)) for x, y in points]
        except (TypeError, ValueError):
            raise GstarkError(f'Curve: {what} are pairs (x, y) of integers') from None
        for pt in points:
            if not self.contains(pt):
                raise GstarkError(f'Curve: {pt} is not on the curve')
        return points, len(points)

    def containsMany(self, points):
        """contains(point) for every row of a device Matrix of count x 2, or for every (x, y) of a list: a list of bools"""
        f = self.field
        if not isinstance(points, Matrix):
            points = [tuple(pt) for pt in points]
            if any(len(pt) != 2 for pt in points):
                raise GstarkError('Curve: points are pairs (x, y) of integers')
        elif points.colCount != 2:
            raise GstarkError(f'Curve: a matrix of points has 2 columns (x, y), not {points.colCount}')
        count = points.rowCount if isinstance(points, Matrix) else len(points)
        if count > MAX_COUNT:
            raise GstarkError(f'Curve: at most 2^20 points per call, not {count}')
        if not count:
            return []
        if not self.onDevice:
            rows = points.toValues() if isinstance(points, Matrix) else points
            return [self.contains((int(x), int(y))) for x, y in rows]
        be = f.backend
        if not isinstance(points, Matrix):
            if any(not (0 <= int(v) < f.modulus) for pt in points for v in pt):
                return [self.contains((int(x), int(y))) for x, y in points]      # (a coordinate that is no element: not a device question)
            points = f.newMatrixFrom([list(pt) for pt in points])
        flags = Vector(be, count, element_size=1)
        be.call('gs_curve_contains', f.le(self.a), f.le(self.b), C.c_void_p(points.ptr), count, C.c_void_p(flags.ptr))
        return [bool(v) for v in be.download(flags.ptr, count)]

    def mulMany(self, points, scalars, addends=None, bits=SCALAR_BITS, device=False):
        """addends[k] + (scalars[k] mod 2^bits) * points[k] for every k.  points: a list of (x, y), one (x, y) for all (the fixed-base
        case), or a device Matrix of count x 2 or 1 x 2 — finite points of the curve; scalars: integers in 0 .. 2^256 - 1; addends:
        None, or a list of (x, y) / None (infinity).  Returns a list of (x, y) / None; with device=True
        the count x 2 Matrix of coordinates ((0, 0) at infinity) and the Vector of count flag bytes (1 = infinity), nothing read back."""
        f = self.field
        bits = int(bits)
        if not 1 <= bits <= SCALAR_BITS:
            raise GstarkError(f'Curve: {bits} bits of a scalar are outside 1 .. {SCALAR_BITS}')
        try:
            scalars = [int(k) for k in scalars]
        except (TypeError, ValueError):
            raise GstarkError('Curve: scalars are integers') from None
        if any(not 0 <= k < 1 << SCALAR_BITS for k in scalars):
            raise GstarkError(f'Curve: a scalar is outside 0 .. 2^{SCALAR_BITS} - 1')
        count = len(scalars)
        if count > MAX_COUNT:
            raise GstarkError(f'Curve: at most 2^20 multiplications per call, not {count}')
        points, npoints = self._readPoints(points, 'points')
        if npoints != count and npoints != 1:
            raise GstarkError(f'Curve: {npoints} points and {count} scalars: one point for all, or one each')
        if addends is not None:
            addends = list(addends)
            finite = iter(self._readPoints([pt for pt in addends if pt is not None], 'addends', count)[0])
            addends = [None if pt is None else next(finite) for pt in addends]
            if len(addends) != count:
                raise GstarkError(f'Curve: {len(addends)} addends and {count} scalars: one addend each')
        if not self.onDevice:
            base = points.toValues() if isinstance(points, Matrix) else points
            base = [(int(x), int(y)) for x, y in base]
            mask = (1 << bits) - 1
            out = [self.add(addends[k] if addends is not None else None, self._hostMul(base[k if npoints > 1 else 0], scalars[k] & mask)) for k in range(count)]
            if not device:
                return out
            flags = Vector(f.backend, count, element_size=1)
            if count:
                f.backend.upload(flags.ptr, bytes(pt is None for pt in out))
            return (f.newMatrixFrom([list(pt or (0, 0)) for pt in out]) if count else Matrix(f.backend, 0, 2)), flags
        be = f.backend
        out, flags = Matrix(be, count, 2), Vector(be, count, element_size=1)
        if count:
            src = points if isinstance(points, Matrix) else f.newMatrixFrom([list(pt) for pt in points])
            ks = Vector(be, count * 32, element_size=1)
            be.upload(ks.ptr, b''.join(k.to_bytes(32, 'little') for k in scalars))
            more = more_inf = None
            if addends is not None:
                more = f.newMatrixFrom([list(pt or (0, 0)) for pt in addends])
                if any(pt is None for pt in addends):
                    more_inf = Vector(be, count, element_size=1)
                    be.upload(more_inf.ptr, bytes(pt is None for pt in addends))
            be.call('gs_curve_mul', f.le(self.a), C.c_void_p(src.ptr), npoints, C.c_void_p(ks.ptr), bits, C.c_void_p(more.ptr) if more is not None else None,
                    C.c_void_p(more_inf.ptr) if more_inf is not None else None, count, C.c_void_p(out.ptr), C.c_void_p(flags.ptr))
        if device:
            return out, flags
        if not count:
            return []
        inf = be.download(flags.ptr, count)
        return [None if inf[k] else (x, y) for k, (x, y) in enumerate(out.toValues())]

    def msm(self, points, scalars, bits=SCALAR_BITS, window=0, device=False):
        """sum over k of (scalars[k] mod 2^bits) * points[k]: (x, y), or None for infinity.  points: a list of (x, y) / None (an infinite
        point contributes nothing: it is dropped with its scalar), or a device Matrix of count x 2 finite points; scalars: a list of
        integers in 0 .. 2^256 - 1, or a device Vector of field elements (each element's bytes are the scalar; bits <= 128 for 16-byte
        elements).  window: 0 lets the plan choose (csrc/msm_plan.h), 1 .. 16 forces the bucket method with windows of that many bits.
        With device=True the result is a 1 x 2 Matrix ((0, 0) at infinity) and a Vector of one flag byte (1 = infinity), nothing read
        back."""
        f = self.field
        bits, window = int(bits), int(window)
        if not 1 <= bits <= SCALAR_BITS:
            raise GstarkError(f'Curve: {bits} bits of a scalar are outside 1 .. {SCALAR_BITS}')
        if not 0 <= window <= MAX_WINDOW:
            raise GstarkError(f'Curve: a window of {window} bits is outside 0 .. {MAX_WINDOW}')
        stride = 32
        if isinstance(scalars, Vector):
            stride, count = scalars.elementSize, scalars.length
            if stride not in (16, 32):
                raise GstarkError(f'Curve: scalars are a vector of field elements, not of {stride}-byte entries')
            if bits > 8 * stride:
                raise GstarkError(f'Curve: {bits} bits of a scalar, but the elements of the scalar vector have {8 * stride}')
        else:
            try:
                scalars = [int(k) for k in scalars]
            except (TypeError, ValueError):
                raise GstarkError('Curve: scalars are integers') from None
            if any(not 0 <= k < 1 << SCALAR_BITS for k in scalars):
                raise GstarkError(f'Curve: a scalar is outside 0 .. 2^{SCALAR_BITS} - 1')
            count = len(scalars)
        if not isinstance(points, Matrix):
            points = list(points)
            if len(points) != count:
                raise GstarkError(f'Curve: {len(points)} points and {count} scalars: a term is one of each')
            if any(pt is None for pt in points):
                if isinstance(scalars, Vector):
                    scalars, stride = [int(k) for k in scalars.toValues()], 32
                scalars = [k for k, pt in zip(scalars, points) if pt is not None]
                points = [pt for pt in points if pt is not None]
                count = len(points)
        points, npoints = self._readPoints(points, 'points', count)
        if npoints != count:
            raise GstarkError(f'Curve: {npoints} points and {count} scalars: a term is one of each')
        if count > MAX_COUNT:
            raise GstarkError(f'Curve: at most 2^20 terms per sum, not {count}')
        if not self.sumsOnDevice:
            rows = points.toValues() if isinstance(points, Matrix) else points
            ks = scalars.toValues() if isinstance(scalars, Vector) else scalars
            mask, total = (1 << bits) - 1, None
            for (x, y), k in zip(rows, ks):
                total = self.add(total, self._hostMul((int(x), int(y)), int(k) & mask))
            if not device:
                return total
            if getattr(f, 'backend', None) is None:
                raise GstarkError('Curve: device=True needs a field with a backend')
            flag = Vector(f.backend, 1, element_size=1)
            f.backend.upload(flag.ptr, bytes([total is None]))
            return f.newMatrixFrom([list(total or (0, 0))]), flag
        be = f.backend
        out, flag = Matrix(be, 1, 2), Vector(be, 1, element_size=1)
        src = ks = None
        if count:
            src = points if isinstance(points, Matrix) else f.newMatrixFrom([list(pt) for pt in points])
            ks = scalars
            if not isinstance(scalars, Vector):
                ks = Vector(be, count * 32, element_size=1)
                be.upload(ks.ptr, b''.join(k.to_bytes(32, 'little') for k in scalars))
        be.call('gs_curve_msm', f.le(self.a), C.c_void_p(src.ptr) if count else None, C.c_void_p(ks.ptr) if count else None, stride, bits, count, window,
                C.c_void_p(out.ptr), C.c_void_p(flag.ptr))
        if device:
            return out, flag
        if be.download(flag.ptr, 1)[0]:
            return None
        x, y = out.toValues()[0]
        return x, y

    def sumMany(self, points, device=False):
        """the sum of the points (a list of (x, y) / None, or a device Matrix of count x 2): `msm` with every scalar 1 and one bit"""
        count = points.rowCount if isinstance(points, Matrix) else len(points := list(points))
        return self.msm(points, [1] * count, bits=1, device=device)

    def mul(self, point, scalar):
        """scalar * point"""
        return self.mulMany([tuple(point)], [scalar])[0]

    # ---- compressed points (include/gstark_sqrt.h, csrc/sqrt.hip): x and the parity y & 1
    @property
    def liftsOnDevice(self):
        """the same for `liftX`, `compressMany` and `decompressMany` (gs_curve_lift_x, gs_curve_compress)"""
        return self._has(('gs_field_sqrt', 'gs_curve_lift_x', 'gs_curve_compress', 'gs_field_sqrt_plan'), 'include/gstark_sqrt.h')

    def compress(self, point):
        """(x, y & 1) of a finite point"""
        x, y = point
        return int(x), int(y) & 1

    def decompress(self, x, parity):
        """the point (x, y) with y & 1 == parity, or None where x^3 + a*x + b is not a square; y = 0 answers both parities"""
        p = self.field.modulus
        x = int(x)
        if not 0 <= x < p:
            raise GstarkError('Curve: x is not a canonical element')
        y = host_sqrt(((x * x + self.a) * x + self.b) % p, p)
        if y is None:
            return None
        return x, (p - y if (int(parity) & 1) and y else y)

    def _deviceFlags(self, flags):
        out = Vector(self.field.backend, len(flags), element_size=1)
        if flags:
            self.field.backend.upload(out.ptr, bytes(flags))
        return out

    def liftX(self, xs, parities=None, device=False):
        """the point (x, y) with y & 1 == parities[k] for every x of a list or a device Vector, None where there is none.  parities: None
        (every y even), a list of 0 / 1, or a device Vector of bytes.  Returns a list of (x, y) / None; with device=True the count x 2
        Matrix of coordinates ((0, 0) where there is no point) and the Vector of count flag bytes (1 = a point), nothing read back."""
        f = self.field
        if isinstance(xs, Vector):
            if xs.elementSize != f.elementSize:
                raise GstarkError(f'Curve: xs are a vector of field elements, not of {xs.elementSize}-byte entries')
            count = xs.length
        else:
            try:
                xs = [int(x) for x in xs]
            except (TypeError, ValueError):
                raise GstarkError('Curve: xs are integers') from None
            if any(not 0 <= x < f.modulus for x in xs):
                raise GstarkError('Curve: an x is not a canonical element')
            count = len(xs)
        if isinstance(parities, Vector):
            if parities.elementSize != 1:
                raise GstarkError(f'Curve: parities are a vector of bytes, not of {parities.elementSize}-byte entries')
            nparities = parities.length
        elif parities is not None:
            try:
                parities = [int(b) for b in parities]
            except (TypeError, ValueError):
                raise GstarkError('Curve: parities are 0 or 1') from None
            if any(b not in (0, 1) for b in parities):
                raise GstarkError('Curve: parities are 0 or 1')
            nparities = len(parities)
        if parities is not None and nparities != count:
            raise GstarkError(f'Curve: {nparities} parities and {count} xs: one parity each')
        if count > MAX_COUNT:
            raise GstarkError(f'Curve: at most 2^20 points per call, not {count}')
        if not self.liftsOnDevice:
            xv = xs.toValues() if isinstance(xs, Vector) else xs
            pv = [0] * count if parities is None else (parities.toValues() if isinstance(parities, Vector) else parities)
            out = [self.decompress(x, b) for x, b in zip(xv, pv)]
            if not device:
                return out
            if getattr(f, 'backend', None) is None:
                raise GstarkError('Curve: device=True needs a field with a backend')
            return (f.newMatrixFrom([list(pt or (0, 0)) for pt in out]) if count else Matrix(f.backend, 0, 2)), self._deviceFlags([pt is not None for pt in out])
        be = f.backend
        out, flags = Matrix(be, count, 2), Vector(be, count, element_size=1)
        if count:
            src = xs if isinstance(xs, Vector) else f.newVectorFrom(xs)
            par = parities if isinstance(parities, Vector) or parities is None else self._deviceFlags(parities)
            be.call('gs_curve_lift_x', f.le(self.a), f.le(self.b), C.c_void_p(src.ptr), C.c_void_p(par.ptr) if par is not None else None, count,
                    C.c_void_p(out.ptr), C.c_void_p(flags.ptr))
        if device:
            return out, flags
        if not count:
            return []
        ok = be.download(flags.ptr, count)
        return [(x, y) if ok[k] else None for k, (x, y) in enumerate(out.toValues())]

    def decompressMany(self, xs, parities, device=False):
        """`liftX` with the parities required"""
        if parities is None:
            raise GstarkError('Curve: decompressMany needs the parities')
        return self.liftX(xs, parities, device=device)

    def compressMany(self, points, device=False):
        """(xs, parities) of finite points (a list of (x, y), or a device Matrix of count x 2): two lists; with device=True a Vector of
        elements and a Vector of bytes, nothing read back"""
        f = self.field
        points, count = self._readPoints(points, 'points', 0)
        if count > MAX_COUNT:
            raise GstarkError(f'Curve: at most 2^20 points per call, not {count}')
        if not self.liftsOnDevice:
            rows = points.toValues() if isinstance(points, Matrix) else points
            pairs = [self.compress(pt) for pt in rows]
            if not device:
                return [x for x, _ in pairs], [b for _, b in pairs]
            if getattr(f, 'backend', None) is None:
                raise GstarkError('Curve: device=True needs a field with a backend')
            return f.newVectorFrom([x for x, _ in pairs]), self._deviceFlags([b for _, b in pairs])
        be = f.backend
        xs, parities = Vector(be, count), Vector(be, count, element_size=1)
        if count:
            src = points if isinstance(points, Matrix) else f.newMatrixFrom([list(pt) for pt in points])
            be.call('gs_curve_compress', C.c_void_p(src.ptr), count, C.c_void_p(xs.ptr), C.c_void_p(parities.ptr))
        if device:
            return xs, parities
        return (xs.toValues(), list(be.download(parities.ptr, count))) if count else ([], [])


def curve224(field):
    """The curve of examples/elliptic/pointmul.aa and assembly/lib224.aa (a = p - 3 over 2^224 - 2^96 + 1) with `.G`, the point the
    reference's examples multiply, and `.order`, the order of G."""
    if field.modulus != MODULUS_224:
        raise GstarkError(f'curve224: the curve lives over the field of 2^224 - 2^96 + 1 elements, not {field.modulus}')
    return Curve(field, -3, B_224, G_224, ORDER_224)


# ---- Schnorr signatures in the relation of lib224.aa (VerifySchnorrSignature): s*G = R + h*P --------------------------------------
def _need_base(curve):
    if curve.G is None or curve.order is None:
        raise GstarkError('schnorr: the curve needs a base point G and its order')


def schnorr_public_keys(curve, secrets):
    """secret * G for every secret"""
    _need_base(curve)
    return curve.mulMany(curve.G, [int(x) % curve.order for x in secrets])


def schnorr_sign_many(curve, secrets, nonces, hashes):
    """[(R, s)]: R = nonce * G (on the device), s = (nonce + h * secret) mod order (host integers).  The reference takes h as given."""
    _need_base(curve)
    secrets, nonces, hashes = list(secrets), list(nonces), list(hashes)
    if not len(secrets) == len(nonces) == len(hashes):
        raise GstarkError(f'schnorr_sign_many: {len(secrets)} secrets, {len(nonces)} nonces and {len(hashes)} hashes: a signature is one of each')
    n = curve.order
    points = curve.mulMany(curve.G, [int(k) % n for k in nonces])
    if any(pt is None for pt in points):
        raise GstarkError('schnorr_sign_many: a nonce is a multiple of the order')
    return [(R, (int(k) + int(h) * int(x)) % n) for R, k, h, x in zip(points, nonces, hashes, secrets)]


def _read_signatures(curve, publics, hashes, signatures, who):
    publics, hashes, signatures = [tuple(pt) for pt in publics], [int(h) for h in hashes], [(tuple(R), int(s)) for R, s in signatures]
    if not len(publics) == len(hashes) == len(signatures):
        raise GstarkError(f'{who}: {len(publics)} public keys, {len(hashes)} hashes and {len(signatures)} signatures: a check is one of each')
    if any(not 0 <= v < 1 << SCALAR_BITS for v in hashes + [s for _, s in signatures]):
        raise GstarkError(f'{who}: a hash or an s is outside 0 .. 2^{SCALAR_BITS} - 1')
    return publics, hashes, signatures


def schnorr_verify_many(curve, publics, hashes, signatures):
    """One bool per signature (R, s) of `hashes[k]` under the public key `publics[k]`: s*G == R + h*P, both sides finite.  Two
    multiplication launches (the fixed-base s*G, and h*P with the addend R), then the rows are compared.  A key or an R that is no
    point of the curve fails."""
    _need_base(curve)
    publics, hashes, signatures = _read_signatures(curve, publics, hashes, signatures, 'schnorr_verify_many')
    sound = [curve.contains(P) and curve.contains(R) for P, (R, _) in zip(publics, signatures)]
    left = curve.mulMany(curve.G, [s for _, s in signatures])
    right = curve.mulMany([P if ok else curve.G for P, ok in zip(publics, sound)], hashes, addends=[R if ok else None for (R, _), ok in zip(signatures, sound)])
    return [ok and l is not None and l == r for ok, l, r in zip(sound, left, right)]


def schnorr_verify_batch(curve, publics, hashes, signatures, rng=None):
    """ONE bool for the whole batch: True when every signature (R, s) of `hashes[k]` under `publics[k]` satisfies s*G == R + h*P.  A
    key or an R that is no point of the curve makes the answer False.  Otherwise one random 128-bit z per signature is drawn
    (`rng.getrandbits` when given, else the `secrets` module) and the batch is accepted exactly when
        (sum z*s mod n)*G + sum (-z mod n)*R + sum (-z*h mod n)*P
    is infinity: ONE `Curve.msm` of 2 * count + 1 terms, so at most 2^19 - 1 signatures.
    The check rests on `curve.order` being the PRIME order of the WHOLE group (true of `curve224`): then every R and P is a multiple of
    G, and a batch with a wrong signature passes for at most one value of a z in 2^128.  With a cofactor a point of small order could
    cancel out of the sum.  A False tells nothing about WHICH signature failed: `schnorr_verify_many` does."""
    _need_base(curve)
    publics, hashes, signatures = _read_signatures(curve, publics, hashes, signatures, 'schnorr_verify_batch')
    count = len(publics)
    if count > MAX_BATCH:
        raise GstarkError(f'schnorr_verify_batch: at most 2^19 - 1 signatures per batch, not {count}')
    if not count:
        return True
    nonces = [R for R, _ in signatures]
    if any(len(pt) != 2 for pt in publics + nonces) or not all(curve.containsMany(publics + nonces)):
        return False
    n = curve.order
    zs = [(rng.getrandbits(128) if rng is not None else _secrets.randbits(128)) or 1 for _ in range(count)]
    scalars = [sum(z * s for z, (_, s) in zip(zs, signatures)) % n] + [-z % n for z in zs] + [-z * h % n for z, h in zip(zs, hashes)]
    return curve.msm([tuple(curve.G)] + nonces + publics, scalars, bits=n.bit_length()) is None


def schnorr_inputs(curve, publics, hashes, signatures):
    """(raw, assertions) for lib224.verify_schnorr_signature_air(field, count): raw = [Gx, Gy, s bits, Px, Py, h bits, Rx, Ry] with one
    entry per signature (lib224.ts:169-175), and the assertions of lib224.ts:177-187 per signature j at steps 256*j and 256*j + 255."""
    from .pointmul import STEPS, to_bits
    _need_base(curve)
    publics, hashes, signatures = _read_signatures(curve, publics, hashes, signatures, 'schnorr_inputs')
    G, count = curve.G, len(publics)
    raw = [[G[0]] * count, [G[1]] * count, [to_bits(s) for _, s in signatures], [P[0] for P in publics], [P[1] for P in publics],
           [to_bits(h) for h in hashes], [R[0] for R, _ in signatures], [R[1] for R, _ in signatures]]
    assertions = []
    for j, (P, h, (R, _)) in enumerate(zip(publics, hashes, signatures)):
        first = STEPS * j
        assertions += [{'step': first, 'register': reg, 'value': v} for reg, v in ((0, G[0]), (1, G[1]), (2, 0), (3, 0), (7, P[0]), (8, P[1]), (9, R[0]), (10, R[1]))]
        assertions.append({'step': first + STEPS - 1, 'register': 13, 'value': h % curve.field.modulus})
    return raw, assertions
