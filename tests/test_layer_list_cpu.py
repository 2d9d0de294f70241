"""CPU: csrc/layer_list.h under the host C++ compiler (the header needs no HIP there).  first_run_above -- the one binary search
of the list kernels of optim.hip, prep_weights.hip, train_weights.hip and train_fold.hip -- against a linear scan, exhaustively:
every running-count array of n = 1..6 entries with increments in {0, 1, 2, 3} whose last count is positive (entries without
units included, anywhere), every u below the last count, in both spellings (a plain int array, a member of a row table).
part_of_row against the same kind of scan over every split of up to three parts of 1..3 rows."""
import itertools
import os
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'stereo_rcnn_amd', 'csrc')

PROGRAM = r'''
#include "layer_list.h"
#include <cstdio>

struct Row { double pad; int other, end; };              // the count is a member somewhere inside a wider record

static long checked = 0;

static int scan(const int *end, int n, int u)
{
    for (int i = 0; i < n; ++i)
        if (end[i] > u) return i;
    return -1;
}

static bool arrays(int n, int i, int *end, Row *table)
{
    if (i == n) {
        for (int u = 0; u < end[n - 1]; ++u) {
            const int want = scan(end, n, u);
            const int plain = srcnn::first_run_above(end, n, u), member = srcnn::first_run_above(table, &Row::end, n, u);
            checked += 2;
            if (plain != want || member != want) {
                std::printf("n %d u %d: scan %d, plain array %d, table member %d; counts", n, u, want, plain, member);
                for (int k = 0; k < n; ++k) std::printf(" %d", end[k]);
                std::printf("\n");
                return false;
            }
        }
        return true;
    }
    for (int inc = 0; inc <= 3; ++inc) {
        end[i] = (i ? end[i - 1] : 0) + inc;
        table[i].end = end[i], table[i].other = -1 - end[i], table[i].pad = 0.5;
        if (!arrays(n, i + 1, end, table)) return false;
    }
    return true;
}

int main()
{
    int end[6];
    Row table[6];
    for (int n = 1; n <= 6; ++n)
        if (!arrays(n, 0, end, table)) return 1;
    long parts = 0;
    for (int nparts = 1; nparts <= 3; ++nparts)
        for (int code = 0; code < 27; ++code) {
            const int rows[3] = {1 + code % 3, 1 + code / 3 % 3, 1 + code / 9};
            int row = 0;
            for (int p = 0; p < nparts; ++p)
                for (int r = 0; r < rows[p]; ++r, ++row, ++parts) {
                    int gp = -1, gr = -1;
                    srcnn::part_of_row(nparts, rows, row, gp, gr);
                    if (gp != p || gr != r) {
                        std::printf("part_of_row(%d, {%d, %d, %d}, %d) = (%d, %d), not (%d, %d)\n", nparts, rows[0], rows[1], rows[2], row, gp, gr, p, r);
                        return 1;
                    }
                }
        }
    std::printf("%ld %ld\n", checked, parts);
    return 0;
}
'''


def test_search_and_part_lookup_against_linear_scans(tmp_path):
    cxx = shutil.which('c++')
    assert cxx, 'no host C++ compiler (c++) on PATH: layer_list.h cannot be checked'
    src, exe = tmp_path / 'layer_list.cpp', tmp_path / 'layer_list'
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    # the cases the program must have walked, counted here on their own: two spellings per (array, u)
    searches = 2 * sum(sum(incs) for n in range(1, 7) for incs in itertools.product(range(4), repeat=n))
    parts = sum(sum(rows[:nparts]) for nparts in (1, 2, 3) for rows in itertools.product((1, 2, 3), repeat=3))
    assert searches == 2 * 46422 and r.stdout.split() == [str(searches), str(parts)]
