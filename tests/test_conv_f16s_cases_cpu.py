"""CPU: every case of tests/conv_f16s_cases.py still has the property that earns it its place.  The numbers written beside each case
(`expect`) are recomputed here from the geometry, and the properties the issue of this table names are asserted on them: ragged
against every tile, the K tiles of every split-K slice, the epilogue the case selects, tile boundaries inside the deconv's tap
groups, the FC tile order.  No GPU, no library."""
import pytest

import conv_f16s_cases as cases

TILE_SIDES = (64, 128, 256)


def test_the_plan_list_is_the_launch_table():
    """Sixteen instantiations, as the switch of launch_conv_f16s has them; the order classes partition them and hold the 4-wave big
    tiles in the one-chain class; the vector-epilogue-only instantiations are the 256x256 tiles and the 4-wave 256x128 / 128x256."""
    assert len(cases.PLANS) == len(set(cases.PLANS)) == 16
    assert {p[:2] for p in cases.PLANS} == {(1, 1), (2, 1), (1, 2), (2, 2), (4, 2), (2, 4), (4, 4)}
    assert sorted(sum(cases.ORDER_CLASSES, [])) == sorted(cases.PLANS)
    big4 = [(4, 4, 4, 2), (4, 2, 4, 2), (4, 2, 4, 3), (2, 4, 4, 2), (2, 4, 4, 3)]
    assert set(big4) <= set(cases.ORDER_CLASSES[0]) and [len(c) for c in cases.ORDER_CLASSES] == [8, 6, 2]
    assert sorted(p for p in cases.PLANS if cases.vector_only(p)) == sorted(big4 + [(4, 4, 8, 2)])
    for (mr, nr, waves, stages), (wmr, wnr) in cases.PER_WAVE.items():
        # the waves tile the workgroup tile: (64 mr x 64 nr) / (32 wmr x 32 wnr) per wave
        assert (2 * mr) % wmr == 0 and (2 * nr) % wnr == 0 and (2 * mr // wmr) * (2 * nr // wnr) == waves, (mr, nr, waves)


def test_the_table_has_the_cases_of_the_issue():
    assert list(cases.BY_ID) == ['ragged3x3', 'f32out-res16', 'f32out-res32', 'narrow', 'slice', 'slice8', 'deconv40-y16',
                                 'deconv40-y32', 'deconv6', 'stem131', 'stem130', 'stride2', 'fc']
    shape = lambda c: (c.B, c.H, c.W, c.cin, c.cout, c.k, c.stride, c.pad)
    want = {'ragged3x3': (2, 23, 37, 96, 200, 3, 1, 1), 'f32out-res16': (2, 23, 37, 96, 200, 3, 1, 1),
            'f32out-res32': (2, 23, 37, 96, 200, 3, 1, 1), 'narrow': (1, 9, 11, 64, 20, 1, 1, 0), 'slice': (1, 9, 11, 64, 24, 1, 1, 0),
            'slice8': (2, 12, 21, 64, 72, 3, 1, 1), 'deconv40-y16': (2, 9, 11, 64, 40, 1, 1, 0), 'deconv40-y32': (2, 9, 11, 64, 40, 1, 1, 0),
            'deconv6': (2, 5, 7, 32, 6, 1, 1, 0), 'stem131': (2, 37, 131, 3, 64, 7, 2, 3), 'stem130': (2, 37, 130, 3, 64, 7, 2, 3),
            'stride2': (2, 21, 33, 64, 136, 1, 2, 0), 'fc': (1, 6, 25, 64, 328, 1, 1, 0)}
    assert {c.id: shape(c) for c in cases.CASES} == want
    by = cases.BY_ID
    assert {i: by[i].splits for i in by if by[i].splits} == {'ragged3x3': (3, 4), 'f32out-res16': (3, 4), 'f32out-res32': (3, 4),
                                                             'narrow': (2,)}
    assert (by['ragged3x3'].y_fmt, by['ragged3x3'].res) == (1, 'split16')
    assert (by['f32out-res16'].y_fmt, by['f32out-res16'].res) == (0, 'split16')
    assert (by['f32out-res32'].y_fmt, by['f32out-res32'].res) == (0, 'f32')
    assert (by['slice'].y_fmt, by['slice'].y_cstride, by['slice'].y_coffset) == (0, 36, 4)
    assert (by['slice8'].y_fmt, by['slice8'].y_cstride, by['slice8'].y_coffset, by['slice8'].res, by['slice8'].res_cstride) \
        == (1, 88, 8, 'split16', 80)
    assert (by['deconv40-y16'].y_fmt, by['deconv40-y32'].y_fmt, by['deconv6'].y_fmt, by['narrow'].y_fmt) == (1, 0, 0, 0)
    assert all(by[i].kind == 'deconv' for i in ('deconv40-y16', 'deconv40-y32', 'deconv6'))
    assert all(by[i].kind == 'stem' and by[i].y_fmt == 1 for i in ('stem131', 'stem130'))
    # every launch of the matrix: sixteen instantiations unsplit on every case, and again at each extra splits request
    assert sum(len(cases.launches(c)) for c in cases.CASES) == 16 * (13 + 3 * 2 + 1)


@pytest.mark.parametrize('cid', list(cases.BY_ID))
def test_case_geometry(cid):
    c = cases.BY_ID[cid]
    e = c.expect
    M, N, nkt = cases.gemm(c)
    assert (M, N, nkt) == (e['M'], e['N'], e['nkt'])
    # ragged against every tile height / width of the plan list, except where the table says the side divides
    assert tuple(s for s in TILE_SIDES if M % s == 0) == e['exact_m']
    assert tuple(s for s in TILE_SIDES if N % s == 0) == e['exact_n']
    for mr, nr in {p[:2] for p in cases.PLANS}:
        assert (M % (64 * mr) != 0) == (64 * mr not in e['exact_m']) and (N % (64 * nr) != 0) == (64 * nr not in e['exact_n'])
    # the K tiles of every slice, at every splits value the matrix asks for
    assert sorted(e['slices']) == sorted((1,) + c.splits)
    for s, want in e['slices'].items():
        got = cases.slice_lengths(nkt, s, c.kind == 'deconv')
        assert got == want and sum(got) == nkt and min(got) >= 1, (s, got)
        assert cases.expected_plan((2, 2, 4, 2, s), nkt, c.kind == 'deconv') == (2, 2, 4, 2, len(want))
    # the epilogue
    assert cases.vector_epilogue(c) == e['vector']
    assert [p for p in cases.PLANS if cases.falls_back(c, p)] == ([] if e['vector'] else [p for p in cases.PLANS if cases.vector_only(p)])
    if c.y_fmt == 1:
        cq, ycs, yco, _ = cases.strides(c)
        assert ycs % 8 == 0 and yco % 8 == 0                 # SPLIT16 output alignment (conv_fill_args)
    # the FC tile order
    assert (M < N) == e['m_fast']
    # mode 1: the tile boundaries inside an (i, j) group
    if c.kind == 'deconv':
        assert N == 4 * c.cout and c.res is None and c.k == 1
        assert {bn: cases.boundaries_inside_groups(c, bn) for bn in TILE_SIDES} == e['inside']
    else:
        assert 'inside' not in e


def test_what_each_case_is_there_for():
    """The property in each case's `why`, as numbers."""
    e = {i: c.expect for i, c in cases.BY_ID.items()}
    by = cases.BY_ID
    for i in ('ragged3x3', 'f32out-res16', 'f32out-res32'):
        assert e[i]['exact_m'] == e[i]['exact_n'] == () and e[i]['slices'][4][-1] < e[i]['slices'][4][0] and e[i]['vector']
    assert by['narrow'].cout % 8 != 0 and e['narrow']['slices'][2] == [1, 1] and not e['narrow']['vector']
    assert by['slice'].cout % 8 == 0 and not e['slice']['vector'] and by['slice'].y_coffset + by['slice'].cout < by['slice'].y_cstride
    s8 = by['slice8']
    assert e['slice8']['vector'] and len({s8.cout, s8.y_cstride, s8.res_cstride}) == 3 and 0 < s8.y_coffset \
        and s8.y_coffset + s8.cout < s8.y_cstride and s8.res_cstride > s8.cout
    for i in ('deconv40-y16', 'deconv40-y32'):
        assert e[i]['vector'] and e[i]['inside'][64] and e[i]['inside'][128] and e[i]['N'] <= 256
    assert not e['deconv6']['vector'] and e['deconv6']['N'] <= 64
    assert (by['stem131'].W + 8) % 2 == 1 and (by['stem130'].W + 8) % 2 == 0
    assert by['stride2'].stride == 2 and by['stride2'].H % 2 == 1 and by['stride2'].W % 2 == 1 and e['stride2']['N'] % 64 != 0
    assert e['fc']['m_fast'] and -(-e['fc']['M'] // 64) == 3 and not any(e[i]['m_fast'] for i in e if i != 'fc')
