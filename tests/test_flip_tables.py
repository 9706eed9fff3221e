"""hp_flip_tables_coco (host only): the flip ensemble's COCO tables equal a derivation this test does itself from the limb table and the PAF channel
table as written below (the tables of the PAF parser, csrc/paf_parser.hip), and the literal the header documents."""
import numpy as np
import pytest

from hyperpose_amd import frontend
from hyperpose_amd._lib import HP_ERR_INVALID, HpError

COCO_PAIRS = [(1, 2), (1, 5), (2, 3), (3, 4), (5, 6), (6, 7), (1, 8), (8, 9), (9, 10), (1, 11), (11, 12), (12, 13), (1, 0), (0, 14), (14, 16), (0, 15),
              (15, 17), (2, 16), (5, 17)]
C_PAIRS_NET = [(12, 13), (20, 21), (14, 15), (16, 17), (22, 23), (24, 25), (0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (28, 29), (30, 31), (34, 35),
               (32, 33), (36, 37), (18, 19), (26, 27)]
SWAPS = [(2, 5), (3, 6), (4, 7), (8, 11), (9, 12), (10, 13), (14, 15), (16, 17)]
LITERAL = [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5, 20, 21, 22, 23, 24, 25, 26, 27, 12, 13, 14, 15, 16, 17, 18, 19, 28, 29, 32, 33, 30, 31, 36, 37, 34, 35]


def _derive(conf_channels):
    part = list(range(conf_channels))
    for a, b in SWAPS:
        part[a], part[b] = b, a
    perm, sign = [None] * 38, [None] * 38
    for k, (p1, p2) in enumerate(COCO_PAIRS):
        m = COCO_PAIRS.index((part[p1], part[p2]))  # the limb whose two parts are the mirrored parts
        for comp, s in ((0, -1), (1, 1)):  # x component: negated; y component: kept
            perm[C_PAIRS_NET[k][comp]] = C_PAIRS_NET[m][comp]
            sign[C_PAIRS_NET[k][comp]] = s
    return part, perm, sign


@pytest.mark.parametrize("conf_channels", [18, 19])
def test_tables_equal_the_derivation_and_the_literal(conf_channels):
    conf, perm, sign = frontend.flip_tables_coco(conf_channels)
    part, want_perm, want_sign = _derive(conf_channels)
    assert conf.dtype == np.int32 and perm.dtype == np.int32 and sign.dtype == np.int8
    assert conf.tolist() == part and perm.tolist() == want_perm and sign.tolist() == want_sign
    assert perm.tolist() == LITERAL
    assert conf[0] == 0 and conf[1] == 1 and (conf_channels == 18 or conf[18] == 18)  # nose, neck and the background stay
    # involutions, and a channel keeps its sign under the permutation: what the exact equivariance needs
    assert conf[conf].tolist() == list(range(conf_channels)) and perm[perm].tolist() == list(range(38))
    assert sign[perm].tolist() == sign.tolist()
    x_channels = sorted(c[0] for c in C_PAIRS_NET)
    assert [c for c in range(38) if sign[c] == -1] == x_channels == list(range(0, 38, 2))
    assert all(sign[c] == 1 for c in range(38) if c not in x_channels)


@pytest.mark.parametrize("bad", [17, 20, 0, -1, 38])
def test_other_channel_counts_are_refused(bad):
    with pytest.raises(HpError) as e:
        frontend.flip_tables_coco(bad)
    assert e.value.code == HP_ERR_INVALID and "conf_channels" in str(e.value) and str(bad) in str(e.value)
