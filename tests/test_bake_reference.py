"""The numpy restatement of occlusion baking (tests/bake_reference.py) against the library's host-only calls, without a GPU: the hash by
known answers and against hiprz_bake_set_of, the float32 frame against its float64 evaluation, the cosine table of the C call against
the numpy float64 table, and the table rule of hiprz_bake_set_directions on both.

THE FRAME, measured once over the normals of _normals() (4 096 seeded unit vectors, +-x, +-y, +-z, z = -0.0 and z = -1 exactly, and 512
normals within 1e-3 of -z, where the construction of Frisvad that Duff et al. revise loses its digits): the float32 (t, bt) differ from
the float64 evaluation of the same formulas on the same float32 normal by at most FRAME_DIFFERENCE = 1.09e-7 in a component (measured
1.083e-7), and the float32 triple (t, bt, n) is orthonormal in float64 to FRAME_ORTHONORMAL = 2.99e-7 (measured: |t.bt| 1.56e-7, |t.n|
2.98e-7, |bt.n| 2.59e-7, ||t|^2 - 1| 2.05e-7, ||bt|^2 - 1| 1.87e-7).  Most of the second figure is the normal's: n is a float32
normalized() with ||n|^2 - 1| up to 2.68e-7, and the FLOAT64 frame of those normals already shows 2.25e-7.  Duff et al. report about 1e-7
for this construction, which is the first figure.  The bars are four times those maxima."""
import numpy as np
import pytest

import bake_reference as BR
from rayzath_amd import _abi, bake

FRAME_DIFFERENCE, FRAME_ORTHONORMAL = 1.09e-7, 2.99e-7      # measured maxima (docstring); the bars are 4 x


def test_hash_known_answers_and_set_of(built):
    # the hash of include/hiprz_bake.h worked by hand in Python integers, not through bake_reference
    def by_hand(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    known = {0: 0, 1: 0x688990C0, 2: 0xD1132181, 63: 0xD3A3CC1E, 64: 0xDCE420BA, 0xFFFFFFFF: 0x6768824A, 20261019: 0x336A513A, 0x80000000: 0xCC4B4124}
    for x, want in known.items():
        assert by_hand(x) == want == int(BR.hash32(x)[0]), hex(x)
        assert bake.set_of(x, 0, 64) == want % 64 and bake.set_of(0, x, 7) == want % 7, hex(x)
    pairs = [(0, 0), (1, 0), (0, 1), (5, 5), (63, 20261019), (64, 20261019), (2**27 - 1, 7), (0xFFFFFFFF, 0), (12345, 0xFFFFFFFF), (2**31, 2**31 + 1)]
    for i, seed in pairs:
        want = by_hand((i ^ seed) & 0xFFFFFFFF)
        assert int(BR.hash32((i ^ seed) & 0xFFFFFFFF)[0]) == want, (i, seed)
        assert bake.set_of(i, seed, 1) == 0
        for S in (2, 3, 4, 7, 64):
            assert bake.set_of(i, seed, S) == want % S == int(BR.set_of(i, seed, S)[0]), (i, seed, S)
    assert bake.set_of(5, 5, 3) == 0 and bake.set_of(3, 0, 0) == 0, "i ^ seed == 0 hashes to 0; S == 0 divides nothing"
    many = np.arange(4096)
    sets = BR.set_of(many, 99, 4)
    assert [bake.set_of(int(i), 99, 4) for i in many[:256]] == sets[:256].tolist()
    assert np.bincount(sets, minlength=4).min() > 900, "the sets are used about equally"


def _normals():
    rng = np.random.default_rng(20261020)
    v = rng.normal(size=(4096, 3))
    near_pole = np.concatenate([rng.normal(size=(512, 2)) * 1e-3, -np.ones((512, 1))], -1)
    special = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, -0.0], [1, 0, -0.0], [-0.6, 0.8, 0.0]])
    n = BR.normalized(np.concatenate([v, near_pole, special]).astype(np.float32))
    assert n.dtype == np.float32 and np.signbit(n[-3, 2]) and n[-4, 2] == -1.0
    return n


def test_the_float32_frame_against_its_float64_evaluation():
    n = _normals()
    t, bt = BR.frame(n)
    assert t.dtype == bt.dtype == np.float32
    n64 = n.astype(np.float64)
    t64, bt64 = BR.frame(n64)
    assert t64.dtype == np.float64
    difference = max(np.abs(t - t64).max(), np.abs(bt - bt64).max())
    T, B = t.astype(np.float64), bt.astype(np.float64)
    dot = lambda a, b: (a * b).sum(-1)
    ortho = max(np.abs(dot(T, B)).max(), np.abs(dot(T, n64)).max(), np.abs(dot(B, n64)).max(), np.abs(dot(T, T) - 1).max(), np.abs(dot(B, B) - 1).max())
    print(f"frame over {len(n)} normals: float32 against float64 {difference:.3e}, orthonormality {ortho:.3e}")
    assert difference <= 4 * FRAME_DIFFERENCE and ortho <= 4 * FRAME_ORTHONORMAL
    # the float64 frame of the same normals is orthonormal to the normals' own error: the formulas, not only their roundings
    assert max(np.abs(dot(t64, bt64)).max(), np.abs(dot(t64, n64)).max(), np.abs(dot(bt64, n64)).max()) <= 4 * FRAME_ORTHONORMAL
    # a right-handed frame: t x bt = n
    assert np.abs(np.cross(T, B) - n64).max() <= 4 * FRAME_ORTHONORMAL
    # a rotated unit direction stays inside the query's [0.99, 1.01], from either end of the table's [0.999, 1.001]
    table = BR.cosine_table(64, 2)[..., :3]
    for scale in (np.sqrt(0.999), 1.0, np.sqrt(1.001)):
        d = BR.rotate(n, t, bt, (table[0] * np.float32(scale)).astype(np.float32)[None])
        sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d.dtype == np.float32 and sq.min() >= 0.99 and sq.max() <= 1.01


@pytest.mark.parametrize("K,S", [(16, 1), (16, 3), (32, 4), (64, 4), (128, 3), (256, 2), (1024, 64)])
def test_the_cosine_table_of_the_library_is_the_float64_table(built, K, S):
    got, want = bake.cosine_directions(K, S), BR.cosine_table(K, S)
    assert got.shape == want.shape == (S, K, 4) and got.dtype == np.float32
    worst = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print(f"K = {K}, S = {S}: largest difference {worst:.3e}")
    assert worst <= 2.0**-23
    assert (got[..., 3] == 0).all() and (got[..., 2] > 0).all()
    sq = (got[..., 0] * got[..., 0] + got[..., 1] * got[..., 1]) + got[..., 2] * got[..., 2]
    assert sq.dtype == np.float32 and sq.min() >= 0.999 and sq.max() <= 1.001, "the table would not pass set_directions' unit rule"
    # cosine weighted: the mean of z is 2/3 up to the stratification's 1/K
    assert abs(got[..., 2].astype(np.float64).mean() - 2.0 / 3.0) < 1.0 / K
    if S > 1:
        assert not np.array_equal(got[0], got[1]), "the sets are rotated against each other"


def test_the_cosine_call_refuses_what_set_directions_refuses(built):
    lib = bake.load()
    out = np.full(4 * 16 + 4, 7.0, np.float32)
    for K, S in ((48, 1), (8, 1), (2048, 1), (0, 1), (16, 0), (16, 65)):
        assert lib.hiprz_bake_cosine_directions(K, S, out.ctypes.data) == _abi.ERR_INVALID, (K, S)
    assert lib.hiprz_bake_cosine_directions(16, 1, None) == _abi.ERR_INVALID
    assert (out == 7.0).all(), "a refused call wrote"
    assert lib.hiprz_bake_cosine_directions(16, 1, out.ctypes.data) == _abi.OK and (out[64:] == 7.0).all() and (out[:64] != 7.0).all()
    with pytest.raises(ValueError):
        bake.cosine_directions(48, 1)


def test_the_butterfly_is_a_sum_in_a_fixed_order():
    rng = np.random.default_rng(5)
    for K in (16, 32, 64, 128, 256):
        values = rng.normal(size=(7, K, 3)).astype(np.float32)
        got = BR.butterfly(values)
        exact = values.astype(np.float64).sum(1)
        assert got.dtype == np.float32 and np.abs(got - exact).max() <= K * 2.0**-24 * np.abs(values).sum(1).max()
        ints = rng.integers(-8, 9, size=(7, K, 3)).astype(np.float32)           # small integers add exactly in any order
        assert np.array_equal(BR.butterfly(ints), ints.sum(1))
    assert not np.signbit(BR.butterfly(np.full((1, 16, 3), -0.0, np.float32))).any(), "the lanes start at +0"
