"""CPU checks of the host-side packing of filters (rabitq_amd.pack_filter_bits): the bitmap rq_filter_create reads has bit
(id & 31) of u32 word id >> 5 set for every admitted id."""
import numpy as np
import pytest

from rabitq_amd import pack_filter_bits


def admitted(words, nbits):
    return [i for i in range(nbits) if (int(words[i >> 5]) >> (i & 31)) & 1]


def test_ids_to_words():
    words, nbits = pack_filter_bits(ids=[0, 5, 31, 32, 70, 5])
    assert nbits == 71 and words.dtype == np.uint32 and words.size == 3
    assert words[0] == (1 | 1 << 5 | 1 << 31) and words[1] == 1 and words[2] == 1 << 6
    assert admitted(words, nbits) == [0, 5, 31, 32, 70]


def test_mask_to_words():
    rng = np.random.default_rng(0)
    mask = rng.random(1000) < 0.3
    words, nbits = pack_filter_bits(mask=mask)
    assert nbits == 1000 and words.size == 32
    assert admitted(words, nbits) == list(np.nonzero(mask)[0])
    assert pack_filter_bits(ids=np.nonzero(mask)[0], nbits=1000)[0].tobytes() == words.tobytes()


def test_ids_beyond_nbits_are_dropped():
    words, nbits = pack_filter_bits(ids=np.array([3, 64, 100, 4000], dtype=np.uint32), nbits=65)
    assert nbits == 65 and words.size == 3
    assert admitted(words, nbits) == [3, 64]


def test_empty_set():
    for words, nbits in (pack_filter_bits(ids=[]), pack_filter_bits(ids=np.array([], dtype=np.int64), nbits=0),
                         pack_filter_bits(mask=np.zeros(0, dtype=bool))):
        assert nbits == 0 and words.size == 0
    words, nbits = pack_filter_bits(mask=np.zeros(40, dtype=bool))
    assert nbits == 40 and words.size == 2 and not words.any()


def test_bad_arguments():
    with pytest.raises(ValueError):
        pack_filter_bits()
    with pytest.raises(ValueError):
        pack_filter_bits(ids=[1], mask=[True])
    with pytest.raises(ValueError):
        pack_filter_bits(ids=[-1, 2])
    with pytest.raises(ValueError):
        pack_filter_bits(mask=np.ones(10, dtype=bool), nbits=11)
