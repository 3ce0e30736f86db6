"""The foreign-table images of tests/foreign_codes.py on the host: the builder reproduces the
encoder byte for byte under the encoder's own table; under every foreign table the parser
accepts the image, the oracle's bit-serial decode returns the data, and the batched raw load's
host twin rebuilds the image's gap words.  The damaged images of the GPU tests' negative case
still parse and the oracle refuses them.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import foreign_codes as fc

ALL_CASES = fc.CASES + [(e, None) for e in fc.EDGE]


@pytest.mark.parametrize("r", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("n", [0, 1, 2, 7, 128, 129, 5000, 300_001])
def test_builder_reproduces_the_encoder(gh, orc, r, n):
    d = gh.generate(31 + n, r, n)
    want = gh.encode(d)
    assert np.array_equal(fc.image(orc, gh.parse(want).symbols, d), want)


def test_code_list_is_what_it_says(orc):
    """Kraft sums, length ranges and the incomplete / complete split of the named codes."""
    for code in fc.CODES:
        syms = fc.symbols(orc, code)
        lens = [l for _, l in syms]
        assert lens == sorted(lens) and 1 <= lens[0] and lens[-1] <= 16 and 2 <= len(syms) <= 256
        assert len({s for s, _ in syms}) == len(syms)
        assert (fc.kraft(syms) < 65536) == (code in fc.INCOMPLETE) and fc.kraft(syms) <= 65536
    k = {c: fc.kraft(fc.symbols(orc, c)) / 65536 for c in fc.CODES}
    assert k["k3"] == 0.75 and k["flat8_200"] == 200 / 256 and k["one_and_16"] == 0.5 + 2.0 ** -16
    assert k["holes16"] == 2 / 4 + 3 / 32 + 1 / 512 + 2 / 65536
    assert len({tuple(l for _, l in fc.symbols(orc, f"lengthened_{i}")) for i in range(3)}) == 3


@pytest.mark.parametrize("code,profile", ALL_CASES)
def test_image_parses_decodes_and_resynchronises(gh, orc, code, profile):
    c = fc.case(orc, code, profile)
    s = gh.parse(c.image)
    assert s.symbols == c.symbols and s.n == c.data.size and s.version == 1
    assert s.g == -(-s.w // 4) and gh.lib().gh_stream_validate(ctypes.byref(s.c)) == 0
    if code in fc.EDGE:
        assert s.g == int(code.rsplit("_g", 1)[1])
    else:
        assert s.g % 256 != 0 and 1 << 16 <= s.n <= 1 << 18
    out, total = orc.decode(c.image)
    assert np.array_equal(out, c.data) and total >= s.n
    syms, n, gaps, pay = fc.split(c.image)
    assert syms == c.symbols and n == s.n and pay.size == s.w
    assert np.array_equal(gh.raw_gaps_host(pay, c.symbols), gaps)
    if profile in ("long", "short"):  # the profile is what it says
        assert np.count_nonzero(c.data == c.symbols[-1 if profile == "long" else 0][0]) >= 0.94 * s.n
    if code == "unused_syms":
        assert np.unique(c.data).size == 2


@pytest.mark.parametrize("code", ["k3", "holes16"])
def test_damaged_image_parses_and_the_oracle_refuses_it(gh, orc, code):
    c = fc.case(orc, code)
    bad, i = fc.damage(c.image, c.symbols, c.data)
    assert c.data.size // 2 <= i < c.data.size // 2 + 64
    s = gh.parse(bad)
    good = gh.parse(c.image)
    assert s.symbols == c.symbols and (s.n, s.w, s.g) == (good.n, good.w, good.g)
    assert gh.lib().gh_stream_validate(ctypes.byref(s.c)) == 0
    (_, _, gaps0, pay0), (_, _, gaps1, pay1) = fc.split(c.image), fc.split(bad)
    assert np.array_equal(gaps0, gaps1) and np.array_equal(pay0 | pay1, pay1)  # bits are only set
    words = np.flatnonzero(pay0 != pay1)
    flipped = sum(bin(int(x)).count("1") for x in pay0[words] ^ pay1[words])
    assert 1 <= words.size <= 2 and words[-1] - words[0] <= 1 and 1 <= flipped <= c.symbols[-1][1]
    with pytest.raises(RuntimeError):
        orc.decode(bad)
