"""The Kolmogorov-Smirnov tail beyond 10 000 rows (csrc/rel_ks_large.h) without a GPU: the g++ build of the kernel bodies,
lanes looped, against significance_tests.py ks_2samp_pvalue (scipy's kstwo.sf) on the table of tests/ks_large_cases.py."""
import numpy as np

import emul_rel_ks_large_lib as emul
import ks_large_cases as cases


def test_table_meets_the_bar():
    assert emul.run_length() == cases.RUN
    p, route, left = emul.ks_large_tails(cases.N1, cases.N2, cases.D)
    cases.check(p, route)
    assert left == sum(1 for c in cases.CASES if c[2] == cases.HOST_KS)


def test_a_cell_is_bit_equal_alone_and_inside_a_shuffled_batch():
    order = np.random.default_rng(5).permutation(len(cases.CASES))
    p, route, _ = emul.ks_large_tails(cases.N1[order], cases.N2[order], cases.D[order])
    for pos, i in enumerate(order):
        alone, r, _ = emul.ks_large_tails(cases.N1[i:i + 1], cases.N2[i:i + 1], cases.D[i:i + 1])
        assert r[0] == route[pos] and alone.tobytes() == p[pos:pos + 1].tobytes(), cases.CASES[i]
