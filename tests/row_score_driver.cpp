// Stand-alone driver of csrc/row_score.h for tests/test_row_score_host.py (host compiler, no HIP): the row kernel's and the table
// kernel's order of operations on the CPU, under the header's rule (0) or one of two wrong ones: ties count as greater (1), the
// last maximum wins the value hit (2).  The logarithm is libm's.  Batches until the input ends:
//   rule A n bucket_width n_buckets has_mask
//   n lines: move class ply  policy bits [A]  value bits [3]  mask words [ceil(A / 32)]     (all unsigned decimal, but move/class/ply)
// -> n lines: p_move rank v_label flags bucket cand_mass_bits brier_bits
//    n_buckets lines: six counts, four sum bits
#include <cmath>
#include <cstdio>
#include <vector>

#include "../tamago_amd/csrc/row_score.h"

namespace sc = tg_score;

struct TiesGreaterRule : sc::Rule {
    static bool ahead(float p, int a, float pm, int move) { return p >= pm && a != move; }
};
struct LastMaximumRule : sc::Rule {
    static int value_argmax(float v0, float v1, float v2) {
        int best = 0;
        float m = v0;
        if (v1 >= m) { m = v1; best = 1; }
        if (v2 >= m) { best = 2; }
        return best;
    }
};

static unsigned long long double_bits(double d) {
    unsigned long long u;
    memcpy(&u, &d, 8);
    return u;
}

int main() {
    for (;;) {
        int rule, A, n, bw, nb, has_mask;
        if (scanf("%d", &rule) != 1) return 0;
        if (scanf("%d %d %d %d %d", &A, &n, &bw, &nb, &has_mask) != 5 || rule < 0 || rule > 2 || A < 2 || n < 0 || bw < 1 || nb < 1) return 2;
        const int W = (A + 31) / 32;
        std::vector<sc::RowRecord> rec(n);
        std::vector<float> policy(A);
        std::vector<uint32_t> mask(W);
        for (int r = 0; r < n; ++r) {
            int move, cls, ply;
            float value[3];
            if (scanf("%d %d %d", &move, &cls, &ply) != 3) return 2;
            for (int a = 0; a < A; ++a) {
                unsigned u;
                if (scanf("%u", &u) != 1) return 2;
                policy[a] = sc::bits_float(u);
            }
            for (int k = 0; k < 3; ++k) {
                unsigned u;
                if (scanf("%u", &u) != 1) return 2;
                value[k] = sc::bits_float(u);
            }
            for (int w = 0; w < W; ++w)
                if (scanf("%u", &mask[w]) != 1) return 2;
            const uint32_t *m = has_mask ? mask.data() : nullptr;
            rec[r] = rule == 0   ? sc::score_row<sc::Rule>(policy.data(), value, m, A, move, cls, ply, bw, nb)
                     : rule == 1 ? sc::score_row<TiesGreaterRule>(policy.data(), value, m, A, move, cls, ply, bw, nb)
                                 : sc::score_row<LastMaximumRule>(policy.data(), value, m, A, move, cls, ply, bw, nb);
            printf("%u %d %u %u %d %llu %llu\n", rec[r].p_move, rec[r].rank, rec[r].v_label, rec[r].flags, rec[r].bucket,
                   double_bits(rec[r].cand_mass), double_bits(rec[r].brier));
        }
        for (int b = 0; b < nb; ++b) {
            sc::Bucket acc{};
            sc::reduce_bucket(rec.data(), n, b, acc, [](double x) { return std::log(x); });
            for (int c = 0; c < sc::kCounts; ++c) printf("%llu ", (unsigned long long)acc.count[c]);
            for (int s = 0; s < sc::kSums; ++s) printf("%llu%c", double_bits(acc.sum[s]), s + 1 < sc::kSums ? ' ' : '\n');
        }
    }
}
