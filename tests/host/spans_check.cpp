// The span checker and the section layouts of cw_host.cpp against models, as a stand-alone program for a sanitizer build (make -C gym_craftingworld_amd/csrc
// host_check: g++ -fsanitize=address,undefined; tests/test_spans_host.py builds and runs it).  Exits non-zero, with a line on stderr, on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cw_host.h"

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "spans_check: " __VA_ARGS__); fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); exit(1); } } while (0)

// ---- cwh_spans_clash: every combination of up to two outputs and two inputs at addresses 0 (not given), 8 .. 15 with 0 .. 4 bytes, both flags.  The model of a
// span is the set of byte addresses it covers, a bit each (they lie in 8 .. 18); exactly-sized heap arrays, so that a read past a count is a report.
static const int kPairs = 9 * 5;
static cwh_span pair_span(int p) { const uint64_t a = (uint64_t)(p / 5), b = (uint64_t)(p % 5); return cwh_span{a ? 7 + a : 0, b, 1}; }
static uint32_t byte_set(const cwh_span &s) { return s.at ? (uint32_t)(((1ull << s.bytes) - 1ull) << s.at) : 0u; }

static unsigned long long clash_brute_force()
{
    unsigned long long cases = 0;
    for (int n_outs = 0; n_outs <= 2; n_outs++)
        for (int n_ins = 0; n_ins <= 2; n_ins++) {
            std::vector<cwh_span> outs((size_t)n_outs), ins((size_t)n_ins);
            const int n = n_outs + n_ins;
            long long combos = 1;
            for (int k = 0; k < n; k++) combos *= kPairs;
            for (long long c = 0; c < combos; c++) {
                long long r = c;
                for (int k = 0; k < n; k++, r /= kPairs) (k < n_outs ? outs[(size_t)k] : ins[(size_t)(k - n_outs)]) = pair_span((int)(r % kPairs));
                for (int among = 0; among <= 1; among++, cases++) {
                    int want_o = -1, want_other = -1;
                    for (int o = 0; o < n_outs && want_o < 0; o++) {
                        for (int i = 0; i < n_ins && want_o < 0; i++)
                            if (byte_set(outs[(size_t)o]) & byte_set(ins[(size_t)i])) { want_o = o; want_other = i; }
                        for (int q = o + 1; among && q < n_outs && want_o < 0; q++)
                            if (byte_set(outs[(size_t)o]) & byte_set(outs[(size_t)q])) { want_o = o; want_other = n_ins + q; }
                    }
                    int other = -7;
                    const int got = cwh_spans_clash(outs.data(), n_outs, ins.data(), n_ins, among, &other);
                    CHECK(got == want_o && other == (want_o < 0 ? -7 : want_other), "clash %d outs %d ins combination %lld among %d: (%d, %d), the model says (%d, %d)",
                          n_outs, n_ins, c, among, got, other, want_o, want_other);
                    CHECK(cwh_spans_clash(outs.data(), n_outs, ins.data(), n_ins, among, nullptr) == want_o, "clash without *other, combination %lld", c);
                }
            }
        }
    return cases;
}

// ---- saturation: a span that ends at the top of the address space, or would wrap past it, clashes exactly where cwh_ranges_overlap says
static void saturation()
{
    const uint64_t top = UINT64_MAX;
    const cwh_span s[] = {{top - 15, 15, 1}, {top - 15, 16, 1}, {top - 15, 1000, 1}, {top, 1, 1}, {top, top, 1}, {top - 1, 1, 1}, {16, top, 1}, {16, 16, 1}, {1, top, 1},
                          {top - 16, 1, 1}, {top - 16, 2, 1}};
    const int n = (int)(sizeof(s) / sizeof(s[0]));
    for (int a = 0; a < n; a++)
        for (int b = 0; b < n; b++) {
            const int want = cwh_ranges_overlap(s[a].at, s[a].bytes, s[b].at, s[b].bytes);
            int other = -7;
            CHECK(cwh_spans_clash(&s[a], 1, &s[b], 1, 0, &other) == (want ? 0 : -1) && other == (want ? 0 : -7), "saturation, output %d input %d", a, b);
            const cwh_span two[2] = {s[a], s[b]};
            CHECK(cwh_spans_clash(two, 2, nullptr, 0, 1, &other) == (want ? 0 : -1) && other == (want ? 1 : -7), "saturation, outputs %d and %d", a, b);
            CHECK(cwh_spans_clash(two, 2, nullptr, 0, 0, nullptr) == -1, "outputs are not compared without the flag");
        }
}

static void misaligned()
{
    std::vector<cwh_span> s = {{0, 8, 16}, {32, 8, 16}, {33, 8, 1}, {33, 8, 0}, {34, 8, 2}, {36, 8, 8}, {35, 8, 2}};
    CHECK(cwh_spans_misaligned(s.data(), (int)s.size()) == 5, "the first offender is span 5");
    CHECK(cwh_spans_misaligned(s.data(), 5) == -1 && cwh_spans_misaligned(s.data(), 0) == -1, "no offender among the first five, none among none");
    s[5].at = 0;                                                // (not given: skipped whatever its alignment)
    CHECK(cwh_spans_misaligned(s.data(), (int)s.size()) == 6, "span 6 once span 5 is not given");
    for (uint64_t at = 1; at < 70; at++)
        for (uint64_t align : {1, 2, 4, 16, 3}) {
            const cwh_span one = {at, 0, align};
            CHECK(cwh_spans_misaligned(&one, 1) == (at % align ? 0 : -1), "address %llu alignment %llu", (unsigned long long)at, (unsigned long long)align);
        }
}

// ---- layouts: the general rule, then the visited set and the replay buffer at their largest legal arguments
static void check_layout(const std::vector<uint64_t> &bytes, uint64_t align, const std::vector<uint64_t> &at, uint64_t total, const char *what)
{
    uint64_t sum = 0;
    for (size_t i = 0; i < bytes.size(); i++) {
        CHECK(at[i] == sum && at[i] % align == 0, "%s: section %zu at %llu, not at %llu", what, i, (unsigned long long)at[i], (unsigned long long)sum);
        sum += (bytes[i] + align - 1) / align * align;
    }
    CHECK(total == sum, "%s: %llu bytes, the sections take %llu", what, (unsigned long long)total, (unsigned long long)sum);
}

static void layouts()
{
    for (uint64_t align : {1, 16, 256}) {
        std::vector<uint64_t> bytes = {0, 1, 255, 256, 257, 0, 4096, 17}, at(bytes.size());
        check_layout(bytes, align, at, cwh_sections_layout(bytes.data(), (int)bytes.size(), align, at.data()), "sections");
        CHECK(cwh_sections_layout(bytes.data(), (int)bytes.size(), align, nullptr) == at.back() + (17 + align - 1) / align * align, "sections without offsets");
        CHECK(cwh_sections_layout(nullptr, 0, align, nullptr) == 0, "no sections");
    }
    const int64_t slots = cwh_seen_slots_of(CWH_SEEN_MAX_CAPACITY);
    const uint64_t n = (uint64_t)slots;
    std::vector<uint64_t> at(CWH_SEEN_SECTIONS);
    CHECK(slots == 2 * CWH_SEEN_MAX_CAPACITY, "the largest set has %lld slots", (long long)slots);
    CHECK(cwh_seen_layout(slots, at.data()) == (int64_t)(256 + 48 * n), "the largest set's bytes");
    check_layout({CWH_SEEN_CTL_BYTES, 8 * n, 8 * n, 16 * n, 16 * n}, 16, at, 256 + 48 * n, "seen");
    CHECK(at[CWH_SEEN_S_TAG] == 256 && at[CWH_SEEN_S_OWNER] == 256 + 8 * n && at[CWH_SEEN_S_KEY_A] == 256 + 16 * n && at[CWH_SEEN_S_KEY_B] == 256 + 32 * n, "seen: packed");
    CHECK(cwh_seen_layout(slots, nullptr) == (int64_t)(256 + 48 * n) && cwh_seen_layout(2 * slots, at.data()) == -1 && cwh_seen_layout(slots - 1, nullptr) == -1 &&
          cwh_seen_layout(0, nullptr) == -1 && cwh_seen_layout(1, nullptr) == -1 && cwh_seen_layout(-2, nullptr) == -1 && cwh_seen_layout(INT64_MIN, nullptr) == -1 &&
          cwh_seen_layout(INT64_MAX, nullptr) == -1, "seen: the refused slot counts");

    const int32_t steps[2] = {CWH_REPLAY_MAX_STEPS, 1}, envs[2] = {127, INT32_MAX};       // (steps * num_envs just below 2^31 both ways)
    for (int k = 0; k < 2; k++) {
        const uint64_t N = (uint64_t)envs[k], T = (uint64_t)steps[k] * N;
        std::vector<uint64_t> ra(CWH_REPLAY_SECTIONS);
        const int64_t total = cwh_replay_layout(steps[k], envs[k], ra.data());
        CHECK(total > 0 && total < (1ll << 38) && total == cwh_replay_bytes_of(steps[k], envs[k]), "replay: %lld bytes", (long long)total);
        check_layout({CWH_REPLAY_CTL_BYTES, 4 * N, 16 * T, 16 * T, 16 * T, 16 * T, 16 * T, 16 * T, 4 * T, 4 * T, T, T}, CWH_SNAP_ALIGN, ra, (uint64_t)total, "replay");
    }
    CHECK(cwh_replay_layout(CWH_REPLAY_MAX_STEPS, 128, nullptr) == -1 && cwh_replay_layout(CWH_REPLAY_MAX_STEPS + 1, 1, nullptr) == -1, "replay: past the limits");
}

int main()
{
    const unsigned long long cases = clash_brute_force();
    saturation();
    misaligned();
    layouts();
    printf("ok %llu\n", cases);
    return 0;
}
