// Host-only check of csrc/libstdcxx_sort.hpp, the one restatement of libstdc++'s std::sort that the PAF, PifPaf and PoseProposal parsers
// call on the device: on every sequence below hp::libstdcxx_sort must leave exactly what this machine's std::sort leaves (the libstdc++ the
// oracle is built with), equal keys included -
//   index arrays with key[a] > key[b] (PAF connection candidates, PifPaf annotation scores) and key[a] < key[b] (PoseProposal limbs),
//   24-byte structs sorted in place by a float member (PoseProposal NMS boxes), compared as whole-struct bytes;
// sizes around the 16-element insertion threshold and beyond, keys with mass ties, random floats, all-equal, ascending, descending,
// organ-pipe, and McIlroy-adversary sequences built against this very std::sort, which exhaust the depth limit 2 floor(log2 n) and run
// the heap-sort fall-back (`used_heap`).  Prints "OK <checks>".
#include "../../hyperpose_amd/csrc/libstdcxx_sort.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        ++g_checks;                                              \
        if (!(cond)) {                                           \
            if (++g_fail <= 20) {                                \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                        \
                std::printf("\n");                               \
            }                                                    \
        }                                                        \
    } while (0)

struct box { // ppn_parser.hip's ppn_box
    int grid;
    float conf;
    int x, y, w, h;
};
static_assert(sizeof(box) == 24, "the NMS element");

// M. D. McIlroy, "A Killer Adversary for Quicksort" (1999), played against this std::sort with "less": the comparator decides the values
// lazily so that every pivot lands near an end.  Returned negated, for sorting with "greater" (as oracle/paf_oracle.cpp builds them).
static std::vector<float> killer(int n)
{
    std::vector<int> val(n, n - 1), ptr(n);
    const int gas = n - 1;
    int nsolid = 0, candidate = 0;
    std::iota(ptr.begin(), ptr.end(), 0);
    std::sort(ptr.begin(), ptr.end(), [&](int x, int y) {
        if (val[x] == gas && val[y] == gas) {
            if (x == candidate)
                val[x] = nsolid++;
            else
                val[y] = nsolid++;
        }
        if (val[x] == gas)
            candidate = x;
        else if (val[y] == gas)
            candidate = y;
        return val[x] < val[y];
    });
    std::vector<float> out(n);
    for (int i = 0; i < n; ++i)
        out[i] = (float)(-val[i]);
    return out;
}

// want_heap: -1 = not asserted, 0 / 1 = the heap-sort fall-back must not / must have run (in all three sorts: they see the same answers,
// `<` on the negated keys being `>` on the keys)
static void check(const char* name, const std::vector<float>& key, int want_heap = -1)
{
    const int n = (int)key.size();
    const float* k = key.data();
    std::vector<int> ref(n), got(n);
    bool heap = false;

    std::iota(ref.begin(), ref.end(), 0);
    std::iota(got.begin(), got.end(), 0);
    std::sort(ref.begin(), ref.end(), [k](int a, int b) { return k[a] > k[b]; });
    CHECK(hp::libstdcxx_sort(got.data(), n, [k](int a, int b) { return k[a] > k[b]; }, &heap), "%s >: stack overflow", name);
    CHECK(ref == got, "%s (n = %d): index order with > differs from std::sort", name, n);
    if (want_heap >= 0)
        CHECK(heap == (want_heap != 0), "%s (n = %d) >: used_heap = %d", name, n, (int)heap);

    std::vector<float> neg(n);
    for (int i = 0; i < n; ++i)
        neg[i] = -key[i];
    const float* q = neg.data();
    heap = false;
    std::iota(ref.begin(), ref.end(), 0);
    std::iota(got.begin(), got.end(), 0);
    std::sort(ref.begin(), ref.end(), [q](int a, int b) { return q[a] < q[b]; });
    CHECK(hp::libstdcxx_sort(got.data(), n, [q](int a, int b) { return q[a] < q[b]; }, &heap), "%s <: stack overflow", name);
    CHECK(ref == got, "%s (n = %d): index order with < differs from std::sort", name, n);
    if (want_heap >= 0)
        CHECK(heap == (want_heap != 0), "%s (n = %d) <: used_heap = %d", name, n, (int)heap);

    // the NMS use: whole boxes moved, comparator on a member; every other member distinct, so a wrong permutation of equals shows
    std::vector<box> rb(n), gb;
    for (int i = 0; i < n; ++i)
        rb[i] = box{ i, neg[i], 3 * i, 5 * i + 1, i ^ 0x55, -i };
    gb = rb;
    heap = false;
    std::sort(rb.begin(), rb.end(), [](const box& l, const box& r) { return l.conf < r.conf; });
    CHECK(hp::libstdcxx_sort(gb.data(), n, [](const box& l, const box& r) { return l.conf < r.conf; }, &heap), "%s boxes: stack overflow", name);
    CHECK(n == 0 || std::memcmp(rb.data(), gb.data(), (size_t)n * sizeof(box)) == 0, "%s (n = %d): boxes sorted in place differ from std::sort", name, n);
    if (want_heap >= 0)
        CHECK(heap == (want_heap != 0), "%s (n = %d) boxes: used_heap = %d", name, n, (int)heap);
}

int main()
{
    std::mt19937 rng(5);
    for (int n : { 0, 1, 2, 15, 16, 17, 18, 33, 100, 257, 1000, 4097 }) {
        std::vector<float> key(n);
        for (int rep = 0; rep < 20; ++rep) {
            std::uniform_int_distribution<int> level(0, std::max(2, n / 8) - 1);
            for (float& v : key)
                v = (float)level(rng);
            check("ties", key);
            std::normal_distribution<float> normal;
            for (float& v : key)
                v = normal(rng);
            check("random", key);
        }
        check("all-equal", std::vector<float>(n, 0.25f), 0);
        for (int i = 0; i < n; ++i)
            key[i] = (float)i;
        check("ascending", key, 0);
        for (int i = 0; i < n; ++i)
            key[i] = (float)-i;
        check("descending", key, 0);
        for (int i = 0; i < n; ++i)
            key[i] = (float)std::min(i, n - 1 - i);
        check("organ-pipe", key);
    }
    for (int n : { 17, 40, 200, 1000, 5000 }) {
        std::vector<float> k = killer(n);
        check("killer", k, n >= 40 ? 1 : 0);
        for (float& v : k)
            v = std::floor(v / 3);
        check("killer floored to thirds", k);
    }
    if (g_fail) {
        std::printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    std::printf("OK %d\n", g_checks);
    return 0;
}
