"""Operands that take the rare carries of each field's arithmetic.

Every reduction in csrc/gf128.h, gf128_lazy.h, gf_small.h, gf_wide.h and host_field*.h ends with branches that uniformly random operands
take with probability 2^-32 .. 2^-170: the carry out of the second fold, the closing conditional subtraction, the wrap of the 64-bit
fold.  With C = 2^B - p they are taken by products whose RESIDUE r = a*b mod p is tiny, and any residue can be had on purpose: pick
a != 0 and set b = r * a^-1 mod p.  This module builds such operands for any modulus, names the classes they fall into by predicates on
plain Python integers, and checks a backend's vector members and trace programs on them.

Plain Python, integers only; nothing here is imported from the code under test (check_corner_arithmetic / check_corner_trace take a
backend as an argument and import the package's Python wrappers when they are called).

    corner_cases(p, bits)   {class name: [operand tuples]}     bits = B, the width the modulus is folded at (C = 2^B - p)
    classify_product(p, bits, a, b) / classify_sum(p, bits, a, b)   the predicate classes of one operand pair
    coverage(p, bits)       {predicate class: number of vectors}
    UNREACHABLE             {predicate class: [(applies(p, bits), why)]}: the classes no operand pair reaches for a modulus
"""
import random

MODULUS_128 = 2**128 - 9 * 2**32 + 1
MODULUS_64 = 2**64 - 21 * 2**30 + 1
MODULUS_32 = 2**32 - 3 * 2**25 + 1
MODULUS_17 = 96769
MODULUS_256 = 2**256 - 351 * 2**32 + 1
MODULUS_224 = 2**224 - 2**96 + 1
FIXED = {'p128': (MODULUS_128, 128), 'q64': (MODULUS_64, 64), 'q32': (MODULUS_32, 32), 'q17': (MODULUS_17, 17),
         'p256': (MODULUS_256, 256), 'p224': (MODULUS_224, 224)}
MIN_PER_CLASS = 32

# gf_small.h, q64: four combinations of (carry of s1, carry of s2, wrap of s3, closing subtraction) that steering the RESIDUE alone reaches
# with probability ~2^-24 even among steered operands: a carry of s2 together with a wrap of s3 or a closing subtraction needs
# l2 = (h1 c mod 2^64) within (h2 + 1) c of 2^64 at the same time as s2.  Built backwards instead: h1 = floor(k 2^64 / c) for k = 1 .. 27
# puts l2 just below 2^64; s2 is drawn from [q - k c, 2^64 - k c) (closing subtraction) or [2^64 - k c, l2) (wrap); s1 = s2 - l2 + 2^64;
# lo == h1 2^64 + s1 (mod c), above s1 for a carry of s1 and below it otherwise, hi = (h1 2^64 + s1 - lo) / c; and X = hi 2^64 + lo is
# kept when it factors into a * b with both below q.  The factoring is the slow part, so the operands found are listed here;
# classify_product confirms the combination of each (tests/test_field_corners.py).
Q64_RARE = {
    'q64_0101': [
        (0x70e227bd6b83a622, 0x9371d8d2ed55d3a6), (0x3c5bb7f23cb16958, 0x9d92f00cd49aeb5a), (0x62526332f67df9ed, 0x9119310f81f3609f),
        (0xee2f98e0d14406e7, 0xc7a7186480dfb484), (0xcb4c7a6e497011fb, 0xe9ea0a624986c2be), (0xc2ecb9fac5cec036, 0xc32bac9fd45ea639),
        (0xd7b1442f24301296, 0x42245d400b209eca), (0xff784b1eeffc1833, 0xfb4bbe562f758aee), (0x15b98b97b32605ab, 0x6d728ec8f546330f),
        (0xcf63269524c9372e, 0xfc3ba314508184de), (0xeb6c79376eebda11, 0xbfe53cd24b296c53), (0xfe9f7f77e0418c8b, 0x700efb02a05920ab),
        (0xdf7f6b431f6c8acd, 0x5fbf8b723e045537), (0xcb9298c246e276dc, 0x97d6f4d137408511), (0x2d909e71624b14f8, 0x685dcccf5617e602),
        (0xe3a5abbd33e45e0b, 0xfaacb31d591ad7bb), (0xdd14b44676fdc909, 0x4b48f2b987b1c0c7), (0xeff030bae9d7c71d, 0xedd56285e46f15c6),
        (0xcfdac8def2c31806, 0xf039fc27abb4891a), (0xe1985698c87cefef, 0x73f0083afa5e5221), (0xd5c4d842cbf307bb, 0x215e5cab1f7d17dd),
        (0xe0d85b36f7b20a47, 0xe8a60c81f2ee0b62), (0xbb5488880eee8659, 0x723bf2560f8f0bc4), (0x3448603b0a2d4187, 0xe36415074907356d),
        (0xf2b10928b8654e56, 0xf4eec242a3200172), (0xf9bde3a6f8e9ac0a, 0x854a4a28ecb9c9ee), (0x68255fc043acb3a9, 0xcd79e05aba6af3cc),
        (0xc091b96074331fbf, 0x3dbca1cc234a3e9b), (0xe133849be52b3792, 0x3f596b7547edd6e5), (0x1f46ed838aa9e305, 0x4c0574e5516751d3),
        (0x4baa290eba044e24, 0x1f6caa9727ef9f7f), (0x81cb40b9288ca3b1, 0x24a3701cbc6c031b), (0x8d5b2ab3b0423bb9, 0xdaaba14ee60cf49a),
        (0x383a17d6c28c9eca, 0xa926e545df548381), (0x8ffe97b6624a2aae, 0x7396936e55c8b1d8), (0xed9c099a1429b8e5, 0x500e0882e123fcd3),
    ],
    'q64_0110': [
        (0x8bb6e02b37249054, 0xaa2f429ce6279776), (0xb948f6ccae18a57d, 0xc07de8106acd5031), (0x4120a30df086174e, 0x9208f67a4aa055d9),
        (0x1f34e24bb32f1cc6, 0x4c31699f0ee1f4ed), (0xc9ae61803c549e4b, 0xd436167766601369), (0x9990433398fd1ee, 0xf7bd04335a608264),
        (0xbf408bf7dedea6ec, 0xdfc881ab369aaef0), (0xf49dbbe41a37a6bb, 0x9b8607e442857423), (0x2937ace23bae014d, 0x735fdfcf8e58cbea),
        (0x33c16bf2422c53b0, 0xb7c4024b7dccd5b9), (0xe0f9ce933fa4d205, 0xa919c9858f6c8449), (0x43e8d6643497374b, 0xd21421fd1070563a),
        (0xe773b05ece951b1a, 0xaea46eab33ee9969), (0x5f4723a3359d4c6c, 0xc7a5356a0ac78509), (0xc46bc88b81eb10ae, 0xb5941d6ef352ae8e),
        (0xfbc751f1ed2d86f2, 0xec17ba19074a25d3), (0x946cb337f8c026e5, 0xe046bdac79102cf4), (0xb21cc68302649b91, 0xc83e55b523b60c0d),
        (0xad0770ca53655900, 0xc06274fb691a55c8), (0xf2970121e55f94e6, 0x58367478fef920cc), (0x95adee2af3a307b1, 0x8ef80db2dba7c92d),
        (0x8ed260709114c9cb, 0x4297bd93855097f9), (0x91814164eabf2c56, 0x93121a5852efed43), (0x2baa964427270675, 0xd9ceeaeffaca02a1),
        (0xfa4f081f80533877, 0xda7b12a574143329), (0xa90134842d23538e, 0xe11a87b3c7a59c17), (0xf37119b8478660f3, 0x30d5e7513d7f0b3f),
        (0x614a1a352993daac, 0x61c23b8ca430c663), (0x61013eeff9acffa8, 0x4988bdd2b1e78e0d), (0x6fd400b3498ef38f, 0x3fc97241412168d1),
        (0x66dd10985d943b1c, 0x8ab1210f231c46f1), (0x818909078c0d8efb, 0x807d95dba2edfdaa), (0xc061f8e1c7cc58fa, 0x7b97e96ea433ae93),
        (0xd69fd1b8d547e4ac, 0xc769e6fb135b972e), (0xfb5088d405031ca2, 0x25d835fa77174ab1), (0x72abd7056246fcf6, 0x7c69292c2a947d7a),
    ],
    'q64_1101': [
        (0xafc46a14c4faa206, 0xd871628c3cd6b125), (0x9425de8903d928e9, 0x503f8f7b73c4238a), (0x71ee3fe72a26ebd5, 0xe591aef3e4a70597),
        (0x1fa6893703628eb2, 0xe15f7259e2916c61), (0xc7e294425fc26f4b, 0xd61e3e6b79088e99), (0xb3f00fbb7771880f, 0x842435f33de9cc5b),
        (0xbcc0d833e184f4cb, 0xa3c2c816b63e5a67), (0xd68dfb307522faf5, 0x90115904c03a80a5), (0xb9b596889a3b1010, 0xc00d50bb92c8080f),
        (0xb910ab459253d222, 0xf41cd9a525cd1e7e), (0xd8a671f417ccce6c, 0xc58c89abd4a9699d), (0xdf2f12f33a547157, 0x3544ac9797adb69c),
        (0x37c06749d21819c7, 0xffe4288c0fbb171c), (0x84a1f31f407b5b3c, 0x7d7d6eea66336839), (0x4b02b5c9880f94a7, 0x3f65a249b902f0d7),
        (0xb662bdba7b8940db, 0xf7b2ecc6df730967), (0x761c918e55b7e642, 0xc94fc49137ce60b9), (0xf0cecff9124e1d6d, 0x3b3e60ccec81a191),
        (0xe7707440b187ee55, 0x710290a7d6fdb6cc), (0x4f2cb8194cd02fc4, 0xb4302ad39b2b5d7f), (0x1e0c1561de6b4dd8, 0xed6618f100fe05d6),
        (0xb0f562d11b9fd249, 0xc98c97c33aa184cb), (0xb6fe4c401b78a574, 0x81ef597936d65425), (0xe31ae9ddc2afc763, 0xe6555e90a947d332),
        (0x931606e469dcad09, 0x60fe3fc33cec4425), (0x37ce944ea8c199d4, 0xaa6cc59f1c06b34e), (0x23e69d40dcb71cd3, 0xc6b0dfa6b665e58e),
        (0x73094132c8102d1d, 0xe35ce94ab7311cc1), (0xf45af35d91b1416a, 0x7e7f6f7fe0308c00), (0xae48568b5cb972ff, 0xcca4d123c7db7d31),
        (0x8f642ade7ae8d4ef, 0x637e0cd87ba07f60), (0xcd076af02945a61d, 0xff225e30a3a65514), (0x3175394326640f42, 0x6026c205c9b24251),
        (0xf505411d9e70f0a0, 0x57566e74a0b4ec27), (0x48ae0cb6900796a1, 0x62252183ad374c9f), (0x25cc2525c14d36f0, 0xbcb891ce80a9efed),
    ],
    'q64_1110': [
        (0xbb0c61ed565982df, 0xa540e7753a81aad0), (0x3ca1cf9bcadd5167, 0x75a5954d7db18906), (0xf2ff9a216559e74c, 0xe10dae8a1f649df2),
        (0xf894a6b476a1c5fe, 0x8f7a5c673b832961), (0x49811ed8f001a84c, 0xe26fb53a92ecd274), (0xb2ccf5e6dd93fe6a, 0xba2caf8f4a4c014d),
        (0xe798e4be4873d2ae, 0xcd55264b7412b7ff), (0x767c4404cb564b6a, 0xf0cfcf34b4aef85c), (0x2d1f5483d50cbf1f, 0x9e15bfcb839b0a05),
        (0xa5b63d5aa6eb7067, 0xc8e12a55cfc58bc3), (0xf5039f2794568499, 0xcbcb0807d3536da3), (0x3da5fc4c478a3808, 0x4d2362bd953f6c73),
        (0x71847325fba23c6d, 0xfb59cb6c6612d351), (0xf5d70d48a6cbf88a, 0x570be5fc33a360f7), (0x98cd6e558cbe926e, 0x2eaeab06a197325e),
        (0x3a3826218349524f, 0xcc3435399c841c45), (0xe66a2c7da714f819, 0xf7a9e64c95d49a66), (0x1d2ae56e059ff7f1, 0xf48eed929f477b9d),
        (0x31133696321029aa, 0xc1cd92fd473aab82), (0xed4b8935b4fffd39, 0xdc7146dcde4967c5), (0x25fb56a1a853162b, 0xbbce14442750eff4),
        (0xb68f4e71daf51954, 0xf77675516851fd80), (0x57cf0691db8da9f2, 0xa2787fe93f98829b), (0x55e78ed2f19d511d, 0xf91baaac4b5f1874),
        (0xe00cb680e0e6f55d, 0xf4164dc9dd7229a3), (0x7cbe1fb2673890fc, 0x4c3e7db8a9f2b1e6), (0x8a2553534f2b08af, 0x33a294d64b1edd1e),
        (0x68e94e25d21079fa, 0xf94e292d213859e3), (0xd691d34c3159a6fd, 0x79e51c38a66cff84), (0xfb6e11bd5c969d15, 0xd00cb59c62c60597),
        (0xe2e5f24d9908f5a6, 0x7dc041dd8d8165de), (0xe991856352587f66, 0x32e661a891d6bd5d), (0xc198cc8f48e746ee, 0xe95acef3ad2a6ff0),
        (0x86e7e3ddbdff9946, 0xf6c03837f40895d0), (0xc4eb8b23b6c3887a, 0x90e50bf01b10fe6f), (0xe8e7a90714b17abe, 0xff39847baae6d79d),
    ],
}


def kind_of(p, bits):
    """Which reduction a modulus goes through: 'p128' (gf128.h: shift folds), 'q64' (gf_small.h: three 64-bit folds), 'rem' (gf_small.h
    below 2^32: a 64-bit remainder), 'wide' (gf_wide.h: three limb folds), 'redc' (gf_wide.h, modulus set at run time: two Montgomery
    reductions with R = 2^256)."""
    if (p, bits) == FIXED['p128']:
        return 'p128'
    if (p, bits) == FIXED['q64']:
        return 'q64'
    if (p, bits) in (FIXED['q32'], FIXED['q17']):
        return 'rem'
    if (p, bits) in (FIXED['p256'], FIXED['p224']):
        return 'wide'
    return 'redc'


def carry_bits(p, bits):
    """The width of the word a sum is formed in (a carry out of it is a branch of its own): 64 for the small fields, else the storage."""
    return 64 if bits <= 64 and kind_of(p, bits) != 'redc' else (128 if kind_of(p, bits) == 'p128' else 256)


def edge_list(p, bits):
    """0, 1, 2, p-1, p-2, (p+-1)/2, C, C+-1, p-C, and 2^32k, 2^32k +- 1 for every limb boundary below `bits` (those below p, once each)."""
    c = 2**bits - p
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, c, c - 1, c + 1, p - c]
    for k in range(1, (bits + 31) // 32):
        if 32 * k < bits:
            vals += [2**(32 * k), 2**(32 * k) - 1, 2**(32 * k) + 1]
    out = []
    for v in vals:
        if 0 <= v < p and v not in out:
            out.append(v)
    return out


def product_residues(p, bits, rng):
    """{residue class name: [r]}: the residues the products are steered to."""
    c = 2**bits - p
    fixed_low = [1, 2, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1]
    fixed_top = [p - c - 1, p - c, p - c + 1, p - 2, p - 1]
    out = {'r_fixed_low': sorted({r for r in fixed_low if 0 < r < p}), 'r_fixed_top': sorted({r for r in fixed_top if 0 < r < p})}
    hi = min(p, c << 8)
    out['r_from_C'] = [rng.randrange(c, hi) for _ in range(24)] if c < hi else []              # C <= r < C * 2^8: the carry of fold 2
    out['r_just_above_C'] = [rng.randrange(c, min(p, 2 * c)) for _ in range(24)] if c < p else []   # C <= r < 2C: the wrap of q64's third fold
    out['r_below_C'] = [rng.randrange(1, c) for _ in range(24)] if c > 2 else []                # 1 <= r < C: the closing subtraction
    out['r_top'] = [rng.randrange(max(p - c, 1), p) for _ in range(24)]                         # p - C <= r < p: neither
    return out


def _sqrt_mod(r, p):
    from sympy.ntheory import sqrt_mod
    return sqrt_mod(r, p)


def corner_cases(p, bits, seed=0x636f726e):
    """Named classes of operand tuples for the modulus p folded at width `bits`.  Products and squares are pairs (a, b) whose product has
    a chosen residue; sums and differences are pairs (a, b), both below p."""
    rng = random.Random(seed ^ p)
    c = 2**bits - p
    w = carry_bits(p, bits)
    edges = edge_list(p, bits)
    nz_edges = [e for e in edges if e]
    shared = [rng.randrange(1, p) for _ in range(4)]                       # the same four random a for every residue (scalar forms)
    out = {}
    # ---- products: b = r * a^-1; per residue four random a and four from the edge list (rotating through it)
    turn = 0
    out['mul_zero'] = [(0, 0)] + [(0, e) for e in nz_edges[:12]] + [(e, 0) for e in nz_edges[:12]] + \
                      [(0, rng.randrange(p)) for _ in range(6)] + [(rng.randrange(p), 0) for _ in range(6)]
    residues = product_residues(p, bits, rng)
    for name, rs in residues.items():
        pairs = []
        for r in rs:
            picks = list(shared)
            for _ in range(4):
                picks.append(nz_edges[turn % len(nz_edges)])
                turn += 1
            pairs += [(a, r * pow(a, -1, p) % p) for a in picks]
        out['mul_' + name] = pairs
    # ---- squares: the same residue ranges, those that are quadratic residues, a = b = either root
    ranges = {'r_fixed_low': None, 'r_fixed_top': None, 'r_from_C': (c, min(p, c << 8)), 'r_just_above_C': (c, min(p, 2 * c)), 'r_below_C': (1, c),
              'r_top': (max(p - c, 1), p)}
    for name, span in ranges.items():
        roots = []
        for r in residues[name]:
            s = _sqrt_mod(r, p)
            if s is not None:
                roots += [s, p - s]
        tries = 0
        while span is not None and span[0] < span[1] and len(roots) < MIN_PER_CLASS + 8 and tries < 4096:
            tries += 1
            s = _sqrt_mod(rng.randrange(*span), p)
            if s is not None:
                roots += [s, p - s]
        out['sqr_' + name] = [(s, s) for s in roots]
    out['sqr_edges'] = [(e, e) for e in edges]
    # ---- sums
    targets = [p - 1, p, p + 1, 2**bits - 1, 2**bits, 2**bits + 1, 2**w - 1, 2**w, 2**w + 1, 2 * p - 2]
    sums = []
    for t in dict.fromkeys(targets):
        lo, hi = max(0, t - (p - 1)), min(p - 1, t)
        if lo > hi:
            continue                                                       # not representable with a, b < p
        picks = {lo, hi, (lo + hi) // 2, min(hi, lo + 1), max(lo, hi - 1)} | {rng.randrange(lo, hi + 1) for _ in range(5)}
        picks |= {e for e in edges if lo <= e <= hi}
        sums += [(a, t - a) for a in sorted(picks)]
    out['add_targets'] = sums
    # ---- differences: a - b in {0, +1, -1}, 0 - b, a - (p - 1)
    some = edges + [rng.randrange(p) for _ in range(12)]
    out['sub_near'] = [(a, a - d) for a in some for d in (0, 1, -1) if 0 <= a - d < p]
    out['sub_from_zero'] = [(0, b) for b in some]
    out['sub_p_minus_1'] = [(a, p - 1) for a in some]
    # ---- limb patterns: runs of all-ones 32-bit limbs (the rest zero), paired so that a carry or a borrow runs through every limb
    nl = (max(bits, 1) + 31) // 32
    runs = [(i, j, (2**(32 * j) - 2**(32 * i))) for i in range(nl) for j in range(i + 1, nl + 1)]
    limbs = []
    for i, j, x in runs:
        if x >= p:
            continue
        for y in (1, 2**(32 * i), x, p - 1 - x, (p - x) % p, 2**(32 * i) - 1 if i else 0):
            if 0 <= y < p:
                limbs += [(x, y), (y, x)]
    for j in range(1, nl):                                                 # 2^32j - 2^32i: a borrow through the zero limbs i .. j
        for i in range(j):
            if 2**(32 * j) < p:
                limbs += [(2**(32 * j), 2**(32 * i)), (2**(32 * i), 2**(32 * j)), (2**(32 * j), 1), (0, 2**(32 * i))]
    if not limbs:                                                          # a modulus of one limb: the patterns are the edges themselves
        limbs = [(a, b) for a in edges for b in (1, p - 1)]
    out['limb_patterns'] = limbs
    if kind_of(p, bits) == 'q64':
        for name, pairs in Q64_RARE.items():
            out['mul_' + name] = list(pairs)
    # ---- the runtime flavour: the branches of a Montgomery reduction depend on a * b itself, not on its residue — drawn until each
    # reachable one is taken often enough
    if kind_of(p, bits) == 'redc':
        want = {k: [] for k in ('redc1_sub', 'redc2_sub', 'redc1_keep', 'redc2_keep')}
        pool = nz_edges + [v for pair in out['mul_r_from_C'] + out['mul_r_below_C'] for v in pair]
        for tries in range(20000):
            if all(len(v) >= MIN_PER_CLASS + 8 for k, v in want.items() if not _unreachable(k, p, bits)):
                break
            a = rng.choice(pool) if tries % 3 == 0 else rng.randrange(1, p)
            b = rng.randrange(1, p)
            for k in classify_product(p, bits, a, b):
                if k in want and len(want[k]) < MIN_PER_CLASS + 8:
                    want[k].append((a, b))
        for k, v in want.items():
            out['mul_' + k] = v
    return out


def product_pairs(cases):
    return [pair for name, pairs in cases.items() if name.startswith(('mul_', 'sqr_')) for pair in pairs]


def square_pairs(cases):
    return [pair for name, pairs in cases.items() if name.startswith('sqr_') for pair in pairs]


def sum_pairs(cases):
    return [pair for name, pairs in cases.items() if name.startswith(('add_', 'sub_', 'limb_')) for pair in pairs]


def _redc_flags(t, p):
    """One word-serial Montgomery reduction of t < p * 2^256 (gf_wide.h: gf_redc): (t + m p) / R with m = -t p^-1 mod R; the value
    before the conditional subtraction is below 2p.  -> (result, it reached p, it reached 2^256: the carry limb)."""
    r = 2**256
    m = (-t * pow(p, -1, r)) % r
    u = (t + m * p) >> 256
    return (u - p if u >= p else u), u >= p, u >= r


def classify_product(p, bits, a, b):
    """The predicate classes of the product a * b, written on integers as the headers describe their folds."""
    kind, cls = kind_of(p, bits), []
    x, c, mask = a * b, 2**bits - p, 2**bits - 1
    if kind == 'wide':
        # gf_wide.h fe_mul: fold 1, fold 2, then "fold 3: the carry", then gf_cond_sub_p
        u = (x & mask) + (x >> bits) * c
        v = (u & mask) + (u >> bits) * c
        z = (v & mask) + (v >> bits) * c
        assert z < 2**bits, 'fold 3 carried again'
        cls.append('fold2_carry' if v >> bits else 'fold2_fits')
        cls.append('final_sub' if z >= p else 'final_keep')
    elif kind == 'p128':
        # gf128.h fe_reduce_wide: V = lo + 9 hi 2^32 - hi = (v0..v3) + T 2^128; w + k 2^128 = (v0..v3) + T C; then t = w + C
        hi, lo = x >> 128, x & mask
        v = lo + ((9 * hi) << 32) - hi
        s = (v & mask) + (v >> 128) * c
        k, wv = s >> 128, s & mask
        assert k <= 1
        cls.append('k_set' if k else 'k_clear')
        cls.append('close_overflow' if wv + c >= 2**128 else 'close_keep')
        if k:
            assert wv + c < 2**128, 'k = 1 leaves w tiny'
    elif kind == 'q64':
        # gf_small.h gfs_mul: s1 = l1 + lo, s2 = l2 + s1, s3 = s2 + h2 c, each modulo 2^64
        m = 2**64
        hi, lo = x >> 64, x % m
        h1, l1 = (hi * c) >> 64, (hi * c) % m
        s1 = (l1 + lo) % m
        f1 = s1 < l1
        h1 += f1
        h2, l2 = (h1 * c) >> 64, (h1 * c) % m
        s2 = (l2 + s1) % m
        f2 = s2 < l2
        h2 += f2
        t = h2 * c
        assert t < m
        s3 = (s2 + t) % m
        f3 = s3 < t
        if f3:
            s3 += c
            assert s3 < m
        f4 = s3 >= p
        cls += ['s1_carry' if f1 else 's1_fits', 's2_carry' if f2 else 's2_fits', 's3_wrap' if f3 else 's3_fits',
                'final_sub' if f4 else 'final_keep', 'q64_%d%d%d%d' % (f1, f2, f3, f4)]
    elif kind == 'redc':
        ab, sub1, top1 = _redc_flags(x, p)
        r2 = pow(2, 512, p)
        _, sub2, top2 = _redc_flags(ab * r2, p)
        cls += ['redc1_sub' if sub1 else 'redc1_keep', 'redc2_sub' if sub2 else 'redc2_keep']
        if top1:
            cls.append('redc1_carry_limb')
        if top2:
            cls.append('redc2_carry_limb')
    else:
        cls.append('remainder')
    return cls


def classify_sum(p, bits, a, b):
    """The predicate classes of a + b and a - b."""
    w = carry_bits(p, bits)
    s = a + b
    return ['add_carry_out' if s >= 2**w else ('add_sub_p' if s >= p else 'add_keep'), 'sub_borrow' if a < b else 'sub_keep']


# Classes no operand pair can reach for a modulus, each with its reason.  tests/test_field_corners.py asserts that the generator finds
# NO vector in them and at least MIN_PER_CLASS in every other class: nothing else may be missing.
UNREACHABLE = {
    'add_carry_out': [(lambda p, bits: 2 * p - 2 < 2**carry_bits(p, bits),
                       'two operands below p sum to less than the word the sum is formed in (p224 and every runtime modulus in 2^256; q32, q17 in 2^64)')],
    'redc1_carry_limb': [(lambda p, bits: p < 2**255, 'a modulus below 2^255 keeps (t + m p) / R below 2p <= 2^256: the carry limb of the reduction stays 0')],
    'redc2_carry_limb': [(lambda p, bits: p < 2**255, 'a modulus below 2^255 keeps (t + m p) / R below 2p <= 2^256: the carry limb of the reduction stays 0')],
    'redc1_sub': [(lambda p, bits: p * p < 2**256,
                   'for p^2 < R = 2^256 the reduction reaches p only if t = j p exactly (t + m p = R u, m = R - j), and a product of two nonzero residues of a prime is no multiple of it')],
    'redc2_sub': [(lambda p, bits: p * p < 2**256,
                   'for p^2 < R = 2^256 the reduction reaches p only if t = j p exactly (t + m p = R u, m = R - j), and a product of two nonzero residues of a prime is no multiple of it')],
    'fold_carry': [(lambda p, bits: kind_of(p, bits) == 'rem', 'q32, q17: the product fits 64 bits and is reduced by one remainder, (a * b) % q: nothing is folded')],
    'final_sub': [(lambda p, bits: kind_of(p, bits) == 'rem', 'q32, q17: the remainder (a * b) % q is canonical as it stands: no closing subtraction')],
    # gf_small.h, q64, the combinations (carry of s1, carry of s2, wrap of s3, closing subtraction) with both of the last two:
    'q64_0011': [(lambda p, bits: True, 'a wrapped s3 is tiny (below h2 c), + c keeps it far below q: no closing subtraction after a wrap')],
    'q64_0111': [(lambda p, bits: True, 'a wrapped s3 is tiny (below h2 c), + c keeps it far below q: no closing subtraction after a wrap')],
    'q64_1011': [(lambda p, bits: True, 'a wrapped s3 is tiny (below h2 c), + c keeps it far below q: no closing subtraction after a wrap')],
    'q64_1111': [(lambda p, bits: True, 'a wrapped s3 is tiny (below h2 c), + c keeps it far below q: no closing subtraction after a wrap')],
}


# the rare branches that squares alone must take too (fe_sqr, lz_sqr and the exponentiation chains multiply nothing else)
SQUARE_CLASSES = {'wide': ['fold2_carry', 'final_sub'], 'p128': ['k_set', 'close_overflow'], 'q64': ['s1_carry', 's2_carry', 's3_wrap', 'final_sub']}


def _unreachable(name, p, bits):
    return any(applies(p, bits) for applies, _ in UNREACHABLE.get(name, ()))


def all_classes(p, bits):
    """Every predicate class of the modulus' reduction, reachable or not."""
    kind = kind_of(p, bits)
    prod = {'wide': ['fold2_carry', 'fold2_fits', 'final_sub', 'final_keep'],
            'p128': ['k_set', 'k_clear', 'close_overflow', 'close_keep'],
            'q64': ['s1_carry', 's1_fits', 's2_carry', 's2_fits', 's3_wrap', 's3_fits', 'final_sub', 'final_keep'] +
                   ['q64_%d%d%d%d' % (a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)],
            'redc': ['redc1_sub', 'redc1_keep', 'redc2_sub', 'redc2_keep', 'redc1_carry_limb', 'redc2_carry_limb'],
            'rem': ['remainder', 'fold_carry', 'final_sub']}[kind]
    return prod + ['add_carry_out', 'add_sub_p', 'add_keep', 'sub_borrow', 'sub_keep']


def coverage(p, bits, cases=None):
    """{predicate class: vectors in it}, every class of all_classes(p, bits) present (0 when the generator finds none)."""
    cases = cases or corner_cases(p, bits)
    count = {k: 0 for k in all_classes(p, bits)}
    for a, b in product_pairs(cases):
        for k in classify_product(p, bits, a, b):
            count[k] += 1
    for a, b in sum_pairs(cases):
        for k in classify_sum(p, bits, a, b):
            count[k] += 1
    return count


def hot_product_pairs(p, bits, cases):
    """The product pairs that take a rare branch (for the lanes a kernel may treat differently: every tiled position holds one)."""
    common = {'fold2_fits', 'final_keep', 'k_clear', 'close_keep', 's1_fits', 's2_fits', 's3_fits', 'redc1_keep', 'redc2_keep', 'remainder'}
    hot = [(a, b) for a, b in product_pairs(cases) if any(k not in common and not k.startswith('q64_') for k in classify_product(p, bits, a, b))]
    return hot or product_pairs(cases)


# ---- a backend's vector members on the corners ------------------------------------------------------------------------------------
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 4096 + 3]
_CASES = {}


def cases_for(p, bits):
    if (p, bits) not in _CASES:
        _CASES[(p, bits)] = corner_cases(p, bits)
    return _CASES[(p, bits)]


def bits_for(q):
    """The fold width of a modulus: the fixed flavours' own, a runtime modulus' bit length."""
    for p, bits in FIXED.values():
        if p == q:
            return bits
    return q.bit_length()


def tiled(pairs, n, shift):
    """n pairs cycling through `pairs` from position `shift` on: with every entry a corner, lane 0, lane 63, the first and the last
    element of every 256-thread workgroup and the ragged tail all hold one — and a different one for every shift."""
    return [pairs[(i + shift) % len(pairs)] for i in range(n)]


def check_corner_arithmetic(backend, q):
    """Every vector member of the backend on the corner operands of its modulus, against Python integers."""
    from genstark_amd.field import PrimeField
    f = PrimeField(backend=backend)
    assert f.modulus == q
    bits = bits_for(q)
    cases = cases_for(q, bits)
    inv = lambda v: pow(v, -1, q) if v % q else 0
    vec = f.newVectorFrom
    prods, sums, hot = product_pairs(cases), sum_pairs(cases), hot_product_pairs(q, bits, cases)
    hot_sums = [(a, b) for a, b in sums if a + b >= q or a < b]

    def vv(pairs, tag):
        xs, ys = [a for a, _ in pairs], [b for _, b in pairs]
        vx, vy = vec(xs), vec(ys)
        assert f.mulVectorElements(vx, vy).toValues() == [a * b % q for a, b in pairs], ('mul', tag)
        assert f.addVectorElements(vx, vy).toValues() == [(a + b) % q for a, b in pairs], ('add', tag)
        assert f.subVectorElements(vx, vy).toValues() == [(a - b) % q for a, b in pairs], ('sub', tag)

    # vector with vector: every pair once, then the rare-branch pairs tiled over the lengths where a kernel's tail and seams lie
    vv(prods + sums, 'all')
    for i, n in enumerate(LENGTHS):
        vv(tiled(hot, n, 7 * i), ('hot products', n))
        vv(tiled(hot_sums, n, 5 * i), ('hot sums', n))
    # vector with scalar: the scalar is a, the vector the matching b of every residue steered to with that a
    by_a = {}
    for a, b in prods:
        by_a.setdefault(a, []).append(b)
    groups = sorted(by_a.items(), key=lambda kv: -len(kv[1]))
    for a, bs in groups:
        if len(bs) < 4 and a not in (1, 2, q - 1, q - 2):
            continue
        assert f.mulVectorElements(vec(bs), a).toValues() == [a * b % q for b in bs], ('mul scalar', a)
    add_targets = [q - 1, q, q + 1, 2**bits - 1, 2**bits, 2**bits + 1, 2**carry_bits(q, bits) - 1, 2**carry_bits(q, bits), 2 * q - 2]
    edges = edge_list(q, bits)
    for s in [e for e in edges if e][:10] + [a for a, _ in groups[:2]]:
        bs = sorted({t - s for t in add_targets if 0 <= t - s < q} | {(s + d) % q for d in (0, 1, -1)} | set(edges))
        v = vec(bs)
        assert f.addVectorElements(v, s).toValues() == [(b + s) % q for b in bs], ('add scalar', s)
        assert f.subVectorElements(v, s).toValues() == [(b - s) % q for b in bs], ('sub scalar', s)
    # division: num = r a, den = a, so that the closing product num * den^-1 has the steered residue r
    num, den = [a * b % q * a % q for a, b in prods], [a for a, _ in prods]
    assert f.divVectorElements(vec(num), vec(den)).toValues() == [x * inv(d) % q for x, d in zip(num, den)], 'div'
    for i, n in enumerate(LENGTHS):
        t = tiled([(a * b % q * a % q, a) for a, b in hot], n, 3 * i)
        assert f.divVectorElements(vec([x for x, _ in t]), vec([d for _, d in t])).toValues() == [x * inv(d) % q for x, d in t], ('div', n)
    # inverses and powers
    assert f.invVectorElements(vec(edges)).toValues() == [inv(e) for e in edges], 'inv'
    assert f.expVectorElements(vec(edges), q - 2).toValues() == [inv(e) for e in edges], 'exp p-2'
    roots = [a for a, _ in square_pairs(cases)]
    assert f.expVectorElements(vec(roots), 2).toValues() == [a * a % q for a in roots], 'exp 2'
    for i, n in enumerate(LENGTHS[:-1]):
        t = [a for a, _ in tiled(square_pairs(cases), n, 11 * i)]
        assert f.expVectorElements(vec(t), 2).toValues() == [a * a % q for a in t], ('exp 2', n)
    # linear combinations: a * b + 0 * o and a * b + 1 * o with o = -r + d, so that the accumulation adds a tiny residue to a value near p
    for a, bs in groups[:6]:
        others = [(-(a * b) + (i % 3) - 1) % q for i, b in enumerate(bs)]
        vb, vo = vec(bs), vec(others)
        assert f.combineManyVectors([vb, vo], [a, 0]).toValues() == [a * b % q for b in bs], ('combine many (a, 0)', a)
        assert f.combineManyVectors([vb, vo], [a, 1]).toValues() == [(a * b + o) % q for b, o in zip(bs, others)], ('combine many (a, 1)', a)
    # dot products of length 1 and 2
    step = max(1, len(hot) // 48)
    picks = hot[::step][:48]
    for i, (a, b) in enumerate(picks):
        assert f.combineVectors(vec([a]), vec([b])) == a * b % q, ('dot 1', a, b)
        a2, b2 = picks[(i + 1) % len(picks)]
        assert f.combineVectors(vec([a, a2]), vec([b, b2])) == (a * b + a2 * b2) % q, ('dot 2', a, b, a2, b2)
    # batch inverse: the running product over the first wave is a tiny residue at every element; again with zeros sprinkled in
    # (the kernel leaves them out of the prefix product)
    rng = random.Random(q ^ 0x62696e76)
    c = 2**bits - q
    small = [r for name in ('r_fixed_low', 'r_from_C', 'r_just_above_C', 'r_below_C') for r in product_residues(q, bits, random.Random(q))[name]]
    for zeros in (False, True):
        xs, run = [], 1
        for j in range(257):
            if zeros and j % 5 == 3:
                xs.append(0)
                continue
            r = small[j % len(small)] if j < 128 else rng.randrange(1, q)
            xs.append(r * inv(run) % q)                                    # the running product becomes r
            run = r
        assert all(x or (zeros and j % 5 == 3) for j, x in enumerate(xs))
        assert f.invVectorElements(vec(xs)).toValues() == [inv(x) for x in xs], ('batch inverse', zeros, c)


def corner_trace_air(field, pairs, segment=4):
    """Two registers, r0' = r0 * r1, r1' = r1, one segment per operand pair: the first step of every segment is a corner product."""
    from genstark_amd.air_generic import GenericAir
    return GenericAir(segment * len(pairs), 2, [2, 1], [], lambda r, k: [r[0] * r[1], r[1]], lambda r, n, k: [n[0] - r[0] * r[1], n[1] - r[1]],
                      lambda seed: [seed[0], seed[1]], None, field, segmentLength=segment)


def check_corner_trace(backend, q, segments=64, expect_compiled=False):
    """The generic trace machine on corner products: the device trace (interpreted, or compiled when the backend is set so) equals the
    AIR's host trace and the recurrence on Python integers."""
    from genstark_amd.field import PrimeField
    f = PrimeField(backend=backend)
    bits = bits_for(q)
    hot = hot_product_pairs(q, bits, cases_for(q, bits))
    assert segments >= 16 and segments & (segments - 1) == 0               # 16 segments: where the device runs the transition program
    step = max(1, len(hot) // segments)
    pairs = (hot[::step] + hot)[:segments]
    air = corner_trace_air(f, pairs)
    seeds = [[a, b] for a, b in pairs]
    before = backend.jit_launches if expect_compiled else 0
    trace = air.initProvingContext([], seeds).generateExecutionTrace().toValues()
    want0, want1 = [], []
    for a, b in pairs:
        for i in range(air.segmentLength):
            want0.append(a * pow(b, i, q) % q)
            want1.append(b)
    assert trace == [want0, want1], 'device trace differs from the recurrence on integers'
    assert [list(r) for r in zip(*air.hostTrace(seeds))] == trace
    if expect_compiled:
        assert backend.jit_launches - before >= 1
    return trace
