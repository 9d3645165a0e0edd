"""The unitig model (tests/unitig_model.py) on hand-worked graphs, and its invariants on random ones. The model pins the definition
of include/kmerind_hip.h (kmi_dbg_compact) that the GPU is held to in test_gpu_unitigs.py. CPU only."""
import random


from tests import oracle as orc
from tests import unitig_model as M

c = M.canonical


def _u(reads, k, t=1, exists=False):
    return M.unitigs_from_strings(M.graph_of_reads(reads, k, exists=exists), t)


def test_one_read_is_one_unitig():
    # no (k-1)-mer repeats on either strand: the read itself (it is the smaller of the two strands), 8 k-mers seen once
    assert _u(["ACCGATTGCAGG"], 5) == [("ACCGATTGCAGG", 8, False)]
    # ... given as its reverse complement: the same unitig
    assert _u([M.revcomp("ACCGATTGCAGG")], 5) == [("ACCGATTGCAGG", 8, False)]


def test_snp_bubble_gives_four_unitigs():
    left, right = "GGTCAGTA", "CAGCTTGA"
    got = _u([left + "A" + right, left + "C" + right], 5)
    # the flanks (their k-mers seen twice), and the two arms from the last 4 bases before to the first 4 after the SNP
    assert got == sorted([
        (c("GGTCAGTA"), 8, False), (c("CAGCTTGA"), 8, False),
        (min("AGTAACAGC", M.revcomp("AGTAACAGC")), 5, False), (min("AGTACCAGC", M.revcomp("AGTACCAGC")), 5, False),
    ])
    assert [s for s, _, _ in got] == ["AGTAACAGC", "AGTACCAGC", "CAGCTTGA", "GGTCAGTA"]


def test_tip_and_min_edge_count():
    main = "ACGGTCATGCCTA"
    reads = [main, main, "ACGGTCATT"]   # the last read leaves main after GTCAT with an error base T
    # t = 1: GTCAT branches; the main path splits there, the error k-mer TCATT (stored as AATGA) is a unitig of its own
    assert _u(reads, 5, t=1) == [("AATGA", 1, False), ("ACGGTCAT", 12, False), ("TAGGCATGA", 10, False)]
    # t = 2: the count-1 edge no longer counts; main is one unitig again (9 k-mers x 2 + 4 of the error read)
    assert _u(reads, 5, t=2) == [("AATGA", 1, False), ("ACGGTCATGCCTA", 22, False)]


def test_circle_is_one_circular_unitig_from_its_smallest_kmer():
    circle = "AACTGCGTCAGATTCCTTGAGCATCG"   # 26 bases, no 4-mer repeats on either strand
    reads = [(circle * 3)[i:i + 12] for i in range(0, len(circle), 3)]
    got = _u(reads, 5)
    # from AACTG (the smallest canonical k-mer, stored forward), 26 nodes + k - 1 bases: the last 4 repeat the first 4
    assert got == [("AACTGCGTCAGATTCCTTGAGCATCG" + "AACT", 72, True)]
    # the same circle read on the other strand: the same unitig
    assert _u([M.revcomp(r) for r in reads], 5) == got


def test_poly_a_self_loop():
    # one node AAAAA whose out A and in A lead to itself: a self-loop never links
    assert _u(["AAAAAAAAA"], 5) == [("AAAAA", 5, False)]
    # inside a read: TAAAA's out A leads into AAAAA, whose in end has A (itself) and T: degree 2, no link either way
    assert _u(["CCGTAAAAAAAAGGT"], 5) == [("AAAAA", 4, False), ("AAAAGGT", 3, False), ("CCGTAAAA", 4, False)]


def test_hairpin():
    # GCAACGTTGC is its own reverse complement: AACGT's out end leads to ACGTT = rc(AACGT), a hairpin, which never links
    assert _u(["GCAACGTTGC"], 5) == [("ACGTTGC", 6, False)]


def test_palindromic_node_at_even_k():
    # k = 4: ACGT is its own reverse complement and links to nothing, so the read falls into three unitigs
    assert _u(["TTACGTGG"], 4) == [("ACGT", 1, False), ("CCACG", 2, False), ("CGTAA", 2, False)]


def test_dangling_edge_after_erase():
    g = M.graph_of_reads(["ACCGATTGCAGG"], 5)
    del g[c("GATTG")]
    # CGATT still has its out edge G (degree 1) but the k-mer behind it is no node: no link; same for ATTGC's in end
    assert M.unitigs_from_strings(g) == [("AATCGGT", 3, False), ("ATTGCAGG", 4, False)]


def test_n_neighbour():
    # the second read ends in N after CGATT: its out end has G twice and A C G T once each from the N
    reads = ["ACCGATTGC", "ACCGATTN"]
    assert _u(reads, 5, t=1) == [("AATCGGT", 6, False), ("GATTA", 1, False), ("GATTGC", 2, False)]
    # t = 2: CGATT's out end has only G; but GATTG (stored CAATC) saw that edge once, so it does not link back, and
    # GATTG / ATTGC lose the count-1 edge between them too
    assert _u(reads, 5, t=2) == [("AATCGGT", 6, False), ("ATTGC", 1, False), ("CAATC", 1, False), ("GATTA", 1, False)]


def test_edge_exists_has_no_occurrences():
    assert _u(["ACCGATTGCAGG"], 5, exists=True) == [("ACCGATTGCAGG", 0, False)]


def test_graph_of_reads_matches_the_oracle():
    # the helper that builds the hand-worked graphs is the oracle's node map (N included)
    rng = random.Random(3)
    for k in (5, 7, 8):
        reads = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 30))) for _ in range(30)]
        reads += ["ACGTNACGTAC", "AAAAAAAAAAAAN", "NCCGATTGCAGG"]
        data = "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads)).encode()
        s = orc.kspec(k)
        km, ed = orc.dbg_parse(s, data)
        for exists in (False, True):
            m = orc.DbgMap(s, exists_only=exists)
            m.insert(km, ed)
            keys, cnt = m.export(canonical=True)
            got = {x: [int(v) for v in cnt[i]] for i, x in enumerate(M.decode_keys(keys, k))}
            assert got == M.graph_of_reads(reads, k, exists=exists)


def _check_invariants(nodes, t):
    g = M.Graph(nodes, t)
    for v in nodes:   # links are symmetric
        for end in ("out", "in"):
            r = g.link(v, end)
            if r is not None:
                assert g.link(*r) == (v, end)
    got = g.unitigs()
    k = g.k
    seen = []
    for seq, occ, circ in got:
        n = len(seq) - k + 1
        kms = [c(seq[i:i + k]) for i in range(n)]
        if circ:
            assert seq[:k - 1] == seq[-(k - 1):]
            assert kms[0] == seq[:k] == min(kms)
        else:
            assert seq <= M.revcomp(seq)
        assert occ == sum(nodes[x][8] for x in kms)
        seen += kms
    assert sorted(seen) == sorted(nodes)   # every node in exactly one unitig, once
    assert sum(len(s) - k + 1 for s, _, _ in got) == len(nodes)
    return got


def test_random_graph_invariants():
    rng = random.Random(11)
    for trial in range(12):
        k = rng.choice([4, 5, 6, 7, 9])
        genome = "".join(rng.choice("ACGT") for _ in range(rng.randint(40, 400)))
        reads = []
        for _ in range(rng.randint(5, 60)):
            i = rng.randrange(len(genome))
            r = list(genome[i:i + rng.randint(k, 40)])
            if r and rng.random() < 0.3:
                r[rng.randrange(len(r))] = rng.choice("ACGTN")
            r = "".join(r)
            reads.append(M.revcomp(r.replace("N", "A")) if rng.random() < 0.5 else r)
        reads += ["A" * rng.randint(k, 2 * k)]
        nodes = M.graph_of_reads([r for r in reads if len(r) >= k], k)
        for t in (1, 2):
            _check_invariants(nodes, t)


def test_model_takes_exported_keys():
    s = orc.kspec(33)
    read = "ACCGATTGCAGGTTACGGATCCAGTAGCATGCAAGT"
    km, ed = orc.dbg_parse(s, ("@r\n%s\n+\n%s\n" % (read, "I" * len(read))).encode())
    m = orc.DbgMap(s)
    m.insert(km, ed)
    keys, cnt = m.export(canonical=True)
    assert M.unitigs(keys, cnt, 33) == [(min(read, M.revcomp(read)), len(read) - 32, False)]
    assert (M.encode_kmer(M.decode_keys(keys[:1], 33)[0], 2) == keys[0]).all()
