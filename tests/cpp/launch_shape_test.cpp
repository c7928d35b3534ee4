// launch_shape_test.cpp -- the launchers' shared host pieces (video_stabilizer_amd/csrc/vs_launch.hpp) against restatements, as a stand-alone
// program: tests/test_launch_shape_cpp.py builds it with the address and undefined-behaviour sanitizers and runs it.  No HIP, no library.
// Prints one line per failed check and, at the end, "DONE <checks> <failures>"; the exit status is 1 if any check failed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../video_stabilizer_amd/csrc/vs_launch.hpp"

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        g_checks++;                                                            \
        if (!(cond)) { g_failed++; if (g_failed <= 50) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } \
    } while (0)

// the chunks are contiguous, cover [0, n) exactly once, and none exceeds 65535 (nor is empty)
static void frame_chunks() {
    const int ns[] = {1, 2, 65535, 65536, 131070, 131071};
    for (int n : ns) {
        std::vector<unsigned char> seen((size_t)n, 0);
        int next = 0, calls = 0;
        vsk::for_frame_chunks(n, [&](int first, int count) {
            CHECK(first == next, "n %d: chunk %d starts at %d, not at %d", n, calls, first, next);
            CHECK(count >= 1 && count <= 65535, "n %d: chunk %d holds %d", n, calls, count);
            CHECK(first >= 0 && first <= n && count <= n - first, "n %d: chunk [%d, +%d) leaves [0, n)", n, first, count);
            for (int i = first; i < first + count && i >= 0 && i < n; i++) seen[(size_t)i]++;
            next = first + count;
            calls++;
        });
        CHECK(next == n, "n %d: the chunks end at %d", n, next);
        CHECK(calls == (n + 65534) / 65535, "n %d: %d chunks", n, calls);
        long once = 0;
        for (unsigned char v : seen) once += v == 1;
        CHECK(once == n, "n %d: %ld frames seen exactly once", n, once);
    }
    int calls = 0;
    vsk::for_frame_chunks(0, [&](int, int) { calls++; });
    CHECK(calls == 0, "n 0: %d chunks", calls);
}

// "every row of every frame starts at a byte address divisible by 4", for 2 rows; and today's launcher expression, written out
static void dword_rows() {
    alignas(8) static unsigned char arena[16];
    for (int base = 0; base < 8; base++)
        for (size_t esz = 1; esz <= 2; esz++)
            for (int stride = 1; stride <= 9; stride++)
                for (size_t fs = 0; fs <= 9; fs++)
                    for (int n = 1; n <= 3; n++) {
                        const unsigned char* const ptr = arena + base;
                        bool brute = true;
                        for (int f = 0; f < n; f++)
                            for (int row = 0; row < 2; row++)
                                brute = brute && ((uintptr_t)ptr + ((size_t)f * fs + (size_t)row * (size_t)stride) * esz) % 4 == 0;
                        const bool expr = (((uintptr_t)ptr | ((size_t)stride * esz) | (n > 1 ? fs * esz : 0)) & 3) == 0;
                        const bool got = vsk::rows_on_dwords(ptr, stride, fs, n, esz);
                        CHECK(!got || brute, "base %d esz %zu stride %d fs %zu n %d: yes, but a row is off a dword", base, esz, stride, fs, n);
                        CHECK(got == expr, "base %d esz %zu stride %d fs %zu n %d: %d, the launchers' expression says %d", base, esz, stride, fs, n, (int)got, (int)expr);
                        // (the expression may say no where these few rows happen to fit, never yes where one does not)
                        CHECK(!expr || brute, "base %d esz %zu stride %d fs %zu n %d: the expression says yes, but a row is off a dword", base, esz, stride, fs, n);
                    }
    // a null pointer asks about the strides alone
    CHECK(vsk::rows_on_dwords(nullptr, 4, 0, 1, 1) && !vsk::rows_on_dwords(nullptr, 6, 0, 1, 1) && vsk::rows_on_dwords(nullptr, 6, 0, 1, 2), "strides alone");
}

// exactly (8, 255) and (16, 0 .. 65535)
static void containers() {
    const int bits[] = {0, 8, 10, 16, 32}, maxs[] = {-1, 0, 254, 255, 256, 1023, 65535, 65536};
    for (int b : bits)
        for (int m : maxs) {
            const bool want = (b == 8 && m == 255) || (b == 16 && m >= 0 && m <= 65535);
            CHECK(vsk::container_ok(b, m) == want, "bits %d max_value %d: %d", b, m, (int)vsk::container_ok(b, m));
        }
}

int main() {
    frame_chunks();
    dword_rows();
    containers();
    printf("DONE %ld %ld\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
