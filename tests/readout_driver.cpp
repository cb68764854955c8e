// Stand-alone driver of csrc/readout.h for tests/test_readout_host.py (host compiler, no HIP): every layout the header owns,
// one fact per line - the root record's rows and size at each A, the self-play tail's place, the analysis record's rows, pv
// block and size at each (A, max_depth), the node record's head indices and size, the state words and move kinds, and the
// message of each error flag word given on the command line.
#include <cstdio>
#include <cstdlib>

#include "../tamago_amd/csrc/readout.h"

int main(int argc, char **argv) {
    using namespace tg_readout;
    const size_t As[] = {82, 170, 362, 5, 7};
    const size_t depths[] = {1, 3, 32};
    for (size_t A : As) {
        printf("root %zu %zu", A, root_record_bytes(A));
        for (int k = 0; k < kRootNumRows; ++k) printf(" %s:%zu:%zu", kRootRows[k].name, kRootRows[k].elem_bytes, root_record_offset(k, A));
        printf("\n");
        for (size_t T : {1, 3, 16})
            for (size_t t = 0; t < T; t += 2) printf("tail %zu %zu %zu %zu %zu\n", A, T, t, root_tail_offset(T, A, t), root_records_bytes(T, A));
        for (size_t d : depths) {
            printf("analysis %zu %zu %zu %zu", A, d, analysis_record_bytes(A, d), analysis_pv_offset(A));
            for (int k = 0; k < kAnaNumRows; ++k) printf(" %s:%zu:%zu", kAnaRows[k].name, kAnaRows[k].elem_bytes, analysis_record_offset(k, A));
            printf("\n");
        }
        printf("node %zu %zu\n", A, tg_pool::node_record_offset(tg_pool::kNumArrays, A));
    }
    printf("root_head %d %d %d %d %d\n", kRootChildren, kRootVisits, kRootRawBits, kRootErr, kRootHeadWords);
    printf("analysis_head %d %d %d %d %d\n", kAnaChildren, kAnaVisits, kAnaVsumBits, kAnaErr, kAnaHeadWords);
    printf("analysis_limits %d %d\n", kAnaWaves, kAnaMaxDepth);
    printf("node_head %d %d %d %d %d %d %d %d %d %zu\n", tg_pool::kHeadChildren, tg_pool::kHeadVisits, tg_pool::kHeadVl,
           tg_pool::kHeadVsumBits, tg_pool::kHeadRawBits, tg_pool::kHeadErr, tg_pool::kHeadNumNodes, tg_pool::kHeadPad,
           tg_pool::kNodeHeadWords, tg_pool::kNodeRecordHead);
    printf("tail_struct %zu %zu %zu %zu %zu\n", sizeof(RootTail), offsetof(RootTail, best), offsetof(RootTail, kind),
           offsetof(RootTail, pos), offsetof(RootTail, cursor));
    printf("state %d %d %d %d %d %d\n", kStateFlags, kStatePasses, kStatePlayed, kStateWords, kStateIdle, kStateNeverResign);
    printf("kinds %d %d %d %d %d\n", kMove, kResign, kSecondPass, kMoveLimit, kIdle);
    printf("flags %d %d %d %d\n", kErrPoolFull, kErrRngEmpty, kErrPipeline, kErrReroot);
    for (int i = 1; i + 1 < argc; i += 2)
        printf("error %s %s [%s]\n", argv[i], argv[i + 1], error_text(atoi(argv[i]), (int32_t)strtol(argv[i + 1], nullptr, 0)).c_str());
    return 0;
}
