/* Host consumer of csrc/s3r_cv_live.h (plain C): prints the rule's answer for every (tile, half, tap) of a volume of edge n and
 * batch B, 64 positions per tile as in the class GEMM.  One line per K tile: "<tile> <half> <tap> <dead>".
 * usage: cv_live_dump <n> <B> */
#include <stdio.h>
#include <stdlib.h>

#include "s3r_cv_live.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int n = atoi(argv[1]), B = atoi(argv[2]);
    if (n < 4 || n % 4 != 0 || B < 1) return 2;
    const int rows = n / 4, groups = n / 4, per_group = n * rows;
    const long long total = (long long)B * groups * per_group;
    if (total >= (1ll << 31)) return 2;
    const int tiles = (int)((total + 63) / 64);
    for (int t = 0; t < tiles; ++t) {
        const int first = t * 64;
        const int last = (first + 64 < (int)total ? first + 64 : (int)total) - 1;
        for (int half = 0; half < 2; ++half)
            for (int tw = 0; tw < 3; ++tw)
                printf("%d %d %d %d\n", t, half, tw, s3r_cv_ktile_dead(n, half, tw, first, last, per_group, groups, rows));
    }
    return 0;
}
