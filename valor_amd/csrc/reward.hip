// The caption reward of self-critical sequence training on the device: CIDEr-D + BLEU-4 of every hypothesis row against the reference
// captions of its clip (valor_amd/scst.py states the rules; scorer/cider_scorer.py:119-200, scorer/bleu_scorer.py:202-250 'closest').
// See include/valor_hip.h for the contract and the table format (valor_reward_tables, built by scst.reward_tables), and ngram.h for the
// keys, the tiling, the passes and the arithmetic: this file is that core plus the sum of its two values. ONE workgroup of four waves per
// hypothesis row; a launch of R workgroups scores sample and greedy rows of every group at once. LDS: 35 KB, four workgroups per CU.
#include "common.h"
#include "../../include/valor_hip.h"
#include "ngram.h"

typedef valor_reward_tables RewardTables;          // the one definition: include/valor_hip.h

__global__ __launch_bounds__(NG_THREADS) void caption_reward_kernel(const int64_t* __restrict__ seq, int64_t ld, int L, int64_t eos, int vocab,
                                                                    const int32_t* __restrict__ clip_idx, RewardTables T,
                                                                    double* __restrict__ reward, double* __restrict__ cider,
                                                                    double* __restrict__ bleu) {
    __shared__ NgramLds S;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int c = clip_idx[r];
    int ref0, ref1;
    ng_clip_refs(T, c, ref0, ref1);
    if (ref1 <= ref0) {                                    // no such clip, or a clip without references: no score (block-uniform)
        if (tid == 0) {
            const double nanv = __longlong_as_double(0x7ff8000000000000ll);
            reward[r] = nanv;
            if (cider) cider[r] = nanv;
            if (bleu) bleu[r] = nanv;
        }
        return;
    }
    int k0;
    bool staged;
    const int len = ng_load_row(S, T, seq, ld, L, eos, vocab, ref0, ref1, k0, staged);
    __syncthreads();
    ng_score_slots(S, T, c, ref0, ref1, len);
    __syncthreads();
    ng_norms(S);
    __syncthreads();
    ng_cider(S, T, ref0, ref1, k0, staged, len);
    __syncthreads();
    if (tid == 0) {                                        // combine: reward = CIDEr-D + BLEU-4
        const double cid = ng_cider_total(S, ref0, ref1);
        int correct[4], guess[4];
        const int reflen = ng_correct(S, len, correct, guess);
        double b[4];
        ng_bleu<int>(correct, guess, len, reflen, b);
        reward[r] = cid + b[3];
        if (cider) cider[r] = cid;
        if (bleu) bleu[r] = b[3];
    }
}

extern "C" int valor_caption_reward(void* stream, const int64_t* seq, int64_t ld, int R, int L, int64_t eos, int vocab, const int32_t* clip_idx,
                                    const RewardTables* tables, double* reward, double* cider, double* bleu) {
    if (ng_check_args(seq, ld, R, L, eos, vocab, clip_idx, tables) != VALOR_OK) return VALOR_ERR_ARG;
    if (R == 0) return VALOR_OK;
    if (!reward) return VALOR_ERR_ARG;
    hipLaunchKernelGGL(caption_reward_kernel, dim3(R), dim3(NG_THREADS), 0, (hipStream_t)stream, seq, ld, L, eos, vocab, clip_idx, *tables, reward,
                       cider, bleu);
    return valor_launch_status();
}
