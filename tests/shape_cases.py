"""The k-mer shapes of the (n_words, bits) instantiations beyond three-word DNA / DNA5 and one-word DNA16, shared by
test_gpu_shape_matrix.py, test_gpu_kmer_ops.py and the CPU-side oracle and ABI tests. Test-side only."""
from tests import oracle as orc

ALPHA = {"DNA": orc.DNA, "DNA5": orc.DNA5, "RNA": orc.RNA, "RNA5": orc.RNA5, "DNA16": orc.DNA16}
BITS = {"DNA": 2, "RNA": 2, "DNA5": 3, "RNA5": 3, "DNA16": 4}

# first and last k of <4,2>, <4,3>, <2,4>, <3,4>, <4,4>, then the 3-bit edges: k = 43 is the first with a character across bit
# 128, k = 64 is 192 bits without pad bits
NEW = [(97, "DNA"), (128, "DNA"), (65, "DNA5"), (85, "DNA5"),
       (17, "DNA16"), (32, "DNA16"), (33, "DNA16"), (48, "DNA16"), (49, "DNA16"), (64, "DNA16"),
       (43, "DNA5"), (64, "DNA5")]
# one shape per instantiation of NEW
REDUCED = [(128, "DNA"), (85, "DNA5"), (32, "DNA16"), (48, "DNA16"), (64, "DNA16")]
# every (n_words, bits) pair once below NEW's: with NEW all twelve
OLD = [(31, "DNA"), (63, "DNA"), (96, "DNA"), (21, "DNA5"), (35, "DNA5"), (63, "DNA5"), (16, "DNA16")]

# IUPAC letter -> the letter of its complement (the text-level rule DNA16's nibble bit reversal packs)
IUPAC_COMPLEMENT = dict(zip("ACGTRYKMSWBDHVN", "TGCAYRMKSWVHDBN"))


def n_words(k, alpha):
    return (k * BITS[alpha] + 63) // 64
