// TEST HARNESS -- runs alpharat_amd/csrc/dev_validate.h on the CPU: the terms of a row (val_row_terms, one lane per row in
// k_val_terms) and their sums (val_accumulate), with a loop over the rows where the device has lanes and a reduction. Boards
// of up to 64 cells run the NW = 1 instantiation, larger ones NW = 4, as the library chooses. It is NOT a CPU fallback:
// nothing in alpharat_amd/ loads this file.
#include <cstdint>
#include <cstring>

#include "../../alpharat_amd/csrc/dev_validate.h"

using namespace ar;

namespace {

// Row r: scores at the position s1[r], s2[r], the final scores f1[r], f2[r], target policies pol1 / pol2 [n][5], the ten
// logits [n][10] (P1's five, then P2's) and the predicted values v1 / v2. `terms` (may be null): the row's ValTerms.
template <int NW>
void run(uint64_t n, const float* s1, const float* s2, const float* f1, const float* f2, const float* pol1, const float* pol2,
         const float* logits, const float* v1, const float* v2, ValTerms* terms, ValAcc* acc) {
    std::memset(acc, 0, sizeof *acc);
    for (uint64_t r = 0; r < n; ++r) {
        PosRec<NW> rec;
        std::memset(&rec, 0, sizeof rec);
        rec.st.s1 = s1[r];
        rec.st.s2 = s2[r];
        std::memcpy(rec.res.policy[0], pol1 + r * 5, 20);
        std::memcpy(rec.res.policy[1], pol2 + r * 5, 20);
        RowGame g;
        std::memset(&g, 0, sizeof g);
        g.final1 = f1[r];
        g.final2 = f2[r];
        const ValTerms t = val_row_terms<NW>(rec, g, logits + r * 10, v1[r], v2[r]);
        if (terms) terms[r] = t;
        val_accumulate(*acc, t);
    }
}

}  // namespace

extern "C" {

// sums: the 18 doubles of ValAcc; counts: top1[2], top2[2]. terms: [n] ValTerms (14 four-byte words each) or null.
void vs_run(int nw, uint64_t n, const float* s1, const float* s2, const float* f1, const float* f2, const float* pol1,
            const float* pol2, const float* logits, const float* v1, const float* v2, void* terms, double* sums,
            uint64_t* counts) {
    ValAcc acc;
    if (nw == 1) run<1>(n, s1, s2, f1, f2, pol1, pol2, logits, v1, v2, (ValTerms*)terms, &acc);
    else run<4>(n, s1, s2, f1, f2, pol1, pol2, logits, v1, v2, (ValTerms*)terms, &acc);
    std::memcpy(sums, acc.d, sizeof acc.d);
    std::memcpy(counts, acc.c, sizeof acc.c);
}

int vs_terms_words(void) { return (int)(sizeof(ValTerms) / 4); }

}  // extern "C"
