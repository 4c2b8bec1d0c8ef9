// Runs csrc/bh_query_host.hpp -- the analysis queries' host arithmetic -- on its own (tests/test_query_host_cpu.py compiles and
// runs this with the host compiler) and prints what it computes, one record a line; the test compares the lines with the Python
// side of the project.  argv[1]: the bodies of the Lagrangian select, "r2-bits-in-hex weight" a line.
#include "bh_query_host.hpp"

#include <cinttypes>
#include <cstdio>
#include <limits>

using namespace bh;

namespace {

uint64_t bits_of(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}

void exponents()
{
    const double maxima[] = {0.0, std::numeric_limits<double>::denorm_min(), 2.2250738585072014e-308, 1.0, std::nextafter(2.0, 0.0),
                             2.0, 1.7976931348623157e308};
    const int64_t counts[] = {0, 1, 2, 3, (int64_t)1 << 24, ((int64_t)1 << 24) + 1};
    for (double m : maxima)
        for (int64_t n : counts) {
            const int L = log2_ceil(n);
            int32_t most = 0;
            (void)exponent_fits(0, m, L, &most);
            std::printf("exp %016" PRIx64 " %" PRId64 " %d %d %d", bits_of(m), n, L, (int)plane_exponent(m, L), (int)most);
            for (int32_t e : {most - 1, most, most + 1, (int32_t)-2000, (int32_t)2000}) {
                int32_t again = 0;
                std::printf(" %d:%d", (int)e, exponent_fits(e, m, L, &again) ? 1 : 0);
                if (again != most) std::printf(" at-most-differs");
            }
            std::printf("\n");
        }
}

void edges_case(const char *name, std::initializer_list<double> edges, int32_t nb)
{
    std::vector<double> in(edges), e2;
    const unsigned why = squared_edges(in.data(), nb, 4, e2);
    std::printf("edges %s %u", name, why);
    if (!why)
        for (double s : e2) std::printf(" %016" PRIx64, bits_of(s));
    std::printf("\n");
}

void edges()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    edges_case("unit", {0.0, 1.0}, 1);
    edges_case("small_middle", {0.0, 1e-150, 1.0}, 2);
    edges_case("square_underflows_middle", {0.0, 1e-200, 1.0}, 2);
    edges_case("square_underflows", {0.0, 1e-200}, 1);
    edges_case("square_overflows", {1.0, 1e200}, 1);
    edges_case("negative", {-1.0, 1.0}, 1);
    edges_case("negative_overflowing", {-1e200, 1.0}, 1);
    edges_case("equal", {1.0, 1.0}, 1);
    edges_case("descending", {2.0, 1.0}, 1);
    edges_case("nan", {0.0, nan}, 1);
    edges_case("no_bins", {0.0, 1.0}, 0);
    edges_case("too_many_bins", {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}, 5);
}

// the text a family words a list of edges with, as bh_queries_host.hpp puts it together: edges_fault's, and behind the count's
// the family's limit
void fault_case(const char *name, const std::vector<double> &in, const char *limit_name, int32_t limit)
{
    std::vector<double> e2;
    const char *fault = edges_fault(squared_edges(in.data(), (int32_t)in.size() - 1, limit, e2));
    std::printf("edges_fault %s %s ", limit_name, name);
    if (!fault) std::printf("-\n");
    else if (fault == kEdgesCountFault) std::printf("%s%s = %d\n", fault, limit_name, (int)limit);
    else std::printf("%s\n", fault);
}

void edge_faults()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const struct { const char *name; int32_t limit; } families[] = {{"BH_RADIAL_MAX_BINS", 4096}, {"BH_MODES_MAX_BINS", 4096},
                                                                     {"BH_DISC_MAX_BINS", 1022}};
    for (const auto &f : families) {
        std::vector<double> long_list((size_t)f.limit + 2), longest((size_t)f.limit + 1);
        for (size_t k = 0; k < long_list.size(); ++k) long_list[k] = (double)k;
        for (size_t k = 0; k < longest.size(); ++k) longest[k] = (double)k;
        fault_case("good", {0.0, 1.0}, f.name, f.limit);
        fault_case("longest", longest, f.name, f.limit);
        fault_case("one_edge", {1.0}, f.name, f.limit);
        fault_case("no_edge", {}, f.name, f.limit);
        fault_case("equal", {1.0, 1.0}, f.name, f.limit);
        fault_case("descending", {2.0, 1.0}, f.name, f.limit);
        fault_case("negative", {-1.0, 1.0}, f.name, f.limit);
        fault_case("infinite", {0.0, inf}, f.name, f.limit);
        fault_case("nan", {0.0, nan}, f.name, f.limit);
        fault_case("square_overflows", {0.0, 1e200}, f.name, f.limit);
        fault_case("squares_underflow", {1e-200, 2e-200}, f.name, f.limit);
        fault_case("too_long", long_list, f.name, f.limit);
        // two faults on one edge: the precedence
        fault_case("negative_and_overflowing", {-1e200, 1.0}, f.name, f.limit);
        fault_case("negative_and_descending", {0.0, -1.0}, f.name, f.limit);
        fault_case("too_long_and_nan", std::vector<double>((size_t)f.limit + 2, nan), f.name, f.limit);
    }
}

void points()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double good[] = {0.0, 1.0, -2.0, 3.0}, bad_y[] = {0.0, 1.0, 2.0, nan, inf, 0.0}, bad_x[] = {-inf, 0.0};
    std::printf("points %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", first_nonfinite_point(good, 2),
                first_nonfinite_point(bad_y, 3), first_nonfinite_point(bad_x, 1), first_nonfinite_point(nullptr, 5),
                first_nonfinite_point(bad_y, 1));
}

void select_args()
{
    const uint64_t zero[] = {0}, one[] = {1}, two[] = {1, 2}, twice[] = {3, 5, 3}, wide[] = {1, 256};
    std::vector<uint64_t> many(LagrangianSelect::kMaxFractions + 1);
    for (size_t k = 0; k < many.size(); ++k) many[k] = k;
    const char *why[] = {select_prefix_fault(0, zero, 1), select_prefix_fault(-1, zero, 1), select_prefix_fault(8, zero, 1),
                         select_prefix_fault(1, nullptr, 1), select_prefix_fault(1, two, 0),
                         select_prefix_fault(7, many.data(), (int32_t)many.size()), select_prefix_fault(0, one, 1),
                         select_prefix_fault(0, two, 2), select_prefix_fault(1, wide, 2), select_prefix_fault(2, wide, 2),
                         select_prefix_fault(1, twice, 3), select_prefix_fault(7, many.data(), LagrangianSelect::kMaxFractions)};
    for (const char *w : why) std::printf("select_args %s\n", w ? w : "-");
}

// the histograms {sum w, count}[np][256] a context would return for the prefixes of one round
void select_histograms(const std::vector<uint64_t> &r2, const std::vector<int64_t> &w, int round, const uint64_t *prefix, int np,
                       std::vector<int64_t> &hist)
{
    std::fill(hist.begin(), hist.end(), 0);
    for (size_t i = 0; i < r2.size(); ++i)
        for (int k = 0; k < np; ++k) {
            if (round > 0 && (r2[i] >> (64 - 8 * round)) != prefix[k]) continue;
            const size_t d = (size_t)((r2[i] >> (64 - 8 * (round + 1))) & 255);
            hist[((size_t)k * 256 + d) * 2] += w[i];
            hist[((size_t)k * 256 + d) * 2 + 1] += 1;
        }
}

void select(const char *name, const std::vector<uint64_t> &r2, const std::vector<int64_t> &w)
{
    const double fractions[] = {1e-9, 0.01, 0.5, 0.5, 1.0};
    const int nf = 5;
    LagrangianSelect sel(fractions, nf);
    std::vector<int64_t> hist((size_t)LagrangianSelect::kMaxFractions * 256 * 2);
    while (!sel.done()) {
        const uint64_t *prefix = nullptr;
        const int np = sel.prefixes(&prefix);
        std::printf("select %s round %d", name, (int)sel.round);
        for (int k = 0; k < np; ++k) std::printf(" %" PRIx64, prefix[k]);
        std::printf("\n");
        select_histograms(r2, w, sel.round, prefix, np, hist);
        sel.advance(hist.data());
    }
    double out[nf];
    int64_t count[nf], mass[nf];
    sel.result(out, count, mass);
    for (int f = 0; f < nf; ++f)
        std::printf("select %s result %016" PRIx64 " %" PRId64 " %" PRId64 "\n", name, bits_of(out[f]), count[f], mass[f]);
}

void catalogue()
{
    const uint32_t label[7] = {40, 3, 17, 9, 25, 1, 12}, count[7] = {5, 9, 5, 2, 9, 5, 7};
    int64_t sums[7 * 5];
    for (int k = 0; k < 35; ++k) sums[k] = (int64_t)1000 * (k / 5) + k % 5 - 3;
    std::vector<int64_t> l, c, s;
    catalogue_order(label, count, sums, 7, 5, l, c, s);
    for (int g = 0; g < 7; ++g) {
        std::printf("cat_in %u %u", label[g], count[g]);
        for (int p = 0; p < 5; ++p) std::printf(" %" PRId64, sums[g * 5 + p]);
        std::printf("\ncat_out %" PRId64 " %" PRId64, l[(size_t)g], c[(size_t)g]);
        for (int p = 0; p < 5; ++p) std::printf(" %" PRId64, s[(size_t)g * 5 + p]);
        std::printf("\n");
    }
    catalogue_order(label, count, sums, 0, 5, l, c, s);
    std::printf("cat_empty %zu %zu %zu\n", l.size(), c.size(), s.size());
}

void layout()
{
    alignas(16) static char block[256];
    char *a = nullptr, *b = nullptr, *e = nullptr;
    struct Sixteen { char c[16]; } *c = nullptr;
    struct Seventeen { char c[17]; } *d = nullptr;
    uint32_t *f = nullptr;
    auto parts = {part(&a, 1), part(&b, 3), part(&c, 1), part(&d, 1), part(&f, 5), part(&e, 0)};
    const size_t total = lay_out(parts);
    std::printf("layout_before %d\n", a == nullptr && b == nullptr && c == nullptr && d == nullptr && f == nullptr && e == nullptr);
    const size_t again = lay_out(parts, block);
    std::printf("layout %zu %zu %zu", total, again, (size_t)(reinterpret_cast<uintptr_t>(block) % 16));
    const char *at[] = {a, b, (char *)c, (char *)d, (char *)f, e};
    const size_t bytes[] = {1, 3, 16, 17, 20, 0};
    for (int k = 0; k < 6; ++k) std::printf(" %td:%zu", at[k] - block, bytes[k]);
    std::printf("\ncapacity %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", grown_capacity(0), grown_capacity(1024),
                grown_capacity(1025), grown_capacity(5000, 2048), grown_capacity(100, 4096));
}

}  // namespace

int main(int argc, char **argv)
{
    exponents();
    edges();
    edge_faults();
    points();
    select_args();
    catalogue();
    layout();
    if (argc > 1) {
        std::vector<uint64_t> r2;
        std::vector<int64_t> w;
        std::FILE *in = std::fopen(argv[1], "r");
        if (!in) return 2;
        uint64_t b;
        int64_t m;
        while (std::fscanf(in, "%" SCNx64 " %" SCNd64, &b, &m) == 2) { r2.push_back(b); w.push_back(m); }
        std::fclose(in);
        select("weighted", r2, w);
        std::fill(w.begin(), w.end(), 0);
        select("massless", r2, w);
    }
    return 0;
}
