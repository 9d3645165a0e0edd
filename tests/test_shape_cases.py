"""CPU-side guards of what the shape-matrix GPU tests rest on: the shape lists name every (n_words, bits) instantiation, and the
white-box key generator really inverts the placement hash for keys of several words."""
import numpy as np

from tests import oracle as orc
from tests.shape_cases import ALPHA, BITS, NEW, OLD, REDUCED, n_words
from tests.test_gpu_index import _keys_in_one_placement_bucket, place_hash_np


def test_the_shape_lists_cover_all_twelve_instantiations():
    def pairs(shapes):
        return {(n_words(k, a), BITS[a]) for k, a in shapes}
    assert pairs(OLD + NEW) == {(w, b) for w in (1, 2, 3, 4) for b in (2, 3, 4)}
    assert pairs(REDUCED) == pairs(NEW) - pairs(OLD) == {(4, 2), (4, 3), (2, 4), (3, 4), (4, 4)}
    for k, a in OLD + NEW:
        s = orc.kspec(k, ALPHA[a])
        assert (s.n_words, s.bits_per_char) == (n_words(k, a), BITS[a])


def test_the_one_bucket_helper_inverts_the_placement_hash():
    """the numpy restatement of kmi_device.h place_hash puts the generated keys into the chosen fine bucket (the top 15 of the
    hash's 32 bits); the words above word 0 are as given and the keys are distinct. That the restatement is the device's hash
    is what the GPU tests' per-bucket counts show."""
    for bucket in (0, 4242, 32767):
        for later in ((), (5,), (5, 6, 7), (0xFEDCBA9876543210, 0x0123456789ABCDEF, 0x0000123456789ABC)):
            keys = _keys_in_one_placement_bucket(9000, bucket, later_words=later)
            assert keys.ndim == (2 if later else 1)
            keys = keys.reshape(9000, -1)
            assert keys.shape[1] == 1 + len(later) and np.unique(keys, axis=0).shape[0] == 9000
            assert (place_hash_np(keys) >> np.uint64(17) == bucket).all()
            assert (keys[:, 1:] == np.array(later, dtype=np.uint64).reshape(1, -1)).all()
    # the hash itself on one key, by hand: one word, all zero
    h = 0x9E3779B9
    h = (h * 0x85EBCA6B) & 0xffffffff; h ^= h >> 15
    h = (h * 0xC2B2AE35) & 0xffffffff; h ^= h >> 13
    h = (h * 0x27D4EB2F) & 0xffffffff; h ^= h >> 16
    assert int(place_hash_np(np.zeros((1, 1), dtype=np.uint64))[0]) == h
