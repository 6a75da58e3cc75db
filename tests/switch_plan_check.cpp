// Host check of csrc/ls_switch_plan.h: a plain program with its own main, built by tests/test_switch_plan_cpu.py with
// AddressSanitizer and UndefinedBehaviorSanitizer.
//   switch_plan_check <tests/switch_ledger_c_parent.txt>
// The ledger holds what the setters of the library answered on real handles before there was a table, one call per row:
//   <kind> <dtype> <metric> <placement> <setter> <enable> \t <return code> \t <ls_l2_small_batch()> \t <ls_last_error() or ->
// ls_switch_ask is held to the return code and the message of every row of a handle, row for row; no difference is
// excused. (The "null" rows are the setters' own null checks and the "flip" rows launch counts: not the table's.)
#include <cstdio>
#include <cstring>
#include <string>

#include "ls_switch_plan.h"

template <size_t N>
static int index_of(const char* const (&names)[N], const char* s) {
    for (size_t i = 0; i < N; ++i)
        if (!std::strcmp(names[i], s)) return (int)i;
    return -1;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: switch_plan_check <ledger>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    static const char* const DTYPES[] = {"f32", "f16", "sq8"};  // LS_DTYPE_*
    static const char* const METRICS[] = {"ip", "l2"};          // LS_METRIC_*
    static const char* const PLACES[] = {"single", "sharded", "replicated", "na"};
    static const char* const SETTERS[] = {"f16", "sq8", "subset", "l2", "ivf"};
    int rows = 0, fails = 0, seen[LS_SW_COUNT] = {};
    char line[1024];
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n' || !std::strncmp(line, "null ", 5) || !std::strncmp(line, "flip ", 5)) continue;
        char kind[16], dtype[16], metric[16], place[16], setter[16], want_msg[512] = "";
        int enable = 0, want_rc = 0, l2_after = 0;
        const int got = std::sscanf(line, "%15s %15s %15s %15s %15s %d\t%d\t%d\t%511[^\n]", kind, dtype, metric, place, setter,
                                    &enable, &want_rc, &l2_after, want_msg);
        const int dt = index_of(DTYPES, dtype), me = index_of(METRICS, metric), pl = index_of(PLACES, place),
                  sw = index_of(SETTERS, setter);
        if (got != 9 || dt < 0 || me < 0 || pl < 0 || sw < 0 || (std::strcmp(kind, "ivf") == 0) != (sw == LS_SW_IVF)) {
            std::fprintf(stderr, "FAIL: cannot read the row: %s", line);
            ++fails;
            continue;
        }
        ++rows, ++seen[sw];
        const ls_switch_answer a = ls_switch_ask((ls_switch)sw, me, dt, (ls_switch_place)pl, enable);
        char have_msg[512] = "-";
        if (a.rc != LS_OK) std::snprintf(have_msg, sizeof have_msg, a.fmt, a.fill);
        if (a.rc != want_rc || std::strcmp(have_msg, want_msg)) {
            std::fprintf(stderr, "FAIL %s %s %s %s %s %d: %d \"%s\", the table says %d \"%s\"\n", kind, dtype, metric, place, setter, enable,
                         a.rc, have_msg, want_rc, want_msg);
            ++fails;
        }
        // every message begins with the name the facts give the setter
        const std::string name = ls_switch_facts_of((ls_switch)sw).setter;
        if (a.rc != LS_OK && std::string(have_msg).compare(0, name.size() + 2, name + ": ")) {
            std::fprintf(stderr, "FAIL: \"%s\" does not begin with %s\n", have_msg, name.c_str());
            ++fails;
        }
    }
    std::fclose(f);
    for (int sw = 0; sw < LS_SW_COUNT; ++sw)
        if (seen[sw] < 10) {
            std::fprintf(stderr, "FAIL: only %d rows of switch %d\n", seen[sw], sw);
            ++fails;
        }
    if (fails) {
        std::fprintf(stderr, "%d failures\n", fails);
        return 1;
    }
    std::printf("ok %d table rows\n", rows);
    return 0;
}
