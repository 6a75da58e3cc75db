// Host check of csrc/ls_scan_plan.h (compiled with -fsanitize=address,undefined and run by
// tests/test_geometry_cpu.py): the header alone, without HIP. Reads one case per line and answers one line per case,
// so that the test holds its Python restatement of the launch rules to the code:
//   S L V rowlist rows blocks   ->  tile rows of the SMALL variant, ls_scan_blocks at 256 CUs, the SMALL decision
//   B n L V n_cu                ->  ls_scan_blocks
//   K blocks keff kp_max        ->  the clamped k', the raw k'
#include <cstdio>

#include "ls_scan_plan.h"

int main() {
    char what;
    long long a, b, c, d, e;
    int cases = 0;
    while (std::scanf(" %c", &what) == 1) {
        if (what == 'S' && std::scanf("%lld %lld %lld %lld %lld", &a, &b, &c, &d, &e) == 5) {
            const int L = (int)a, V = (int)b;
            const int tr = ls_scan_tile_rows(L, ls_scan_small_unroll(V, c != 0));
            std::printf("S %d %d %d\n", tr, ls_scan_blocks_lv(d, L, V, 256), (int)ls_scan_is_small(d, (int)e, tr, 1));
        } else if (what == 'B' && std::scanf("%lld %lld %lld %lld", &a, &b, &c, &d) == 4) {
            std::printf("B %d\n", ls_scan_blocks_lv(a, (int)b, (int)c, (int32_t)d));
        } else if (what == 'K' && std::scanf("%lld %lld %lld", &a, &b, &c) == 3) {
            std::printf("K %d %d\n", ls_kprime((int)a, (int)b, (int)c), ls_kprime_raw(b, (int)a));
        } else {
            std::printf("bad case %c\n", what);
            return 1;
        }
        ++cases;
    }
    std::printf("OK %d cases\n", cases);
    return 0;
}
