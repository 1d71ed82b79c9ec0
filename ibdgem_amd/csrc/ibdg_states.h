// ibdg_states.h -- the integer log-domain IBD-state path: what its host twin (ibdg_states_host.cpp), its
// kernel (ibdg_states.hip) and the entry points share.  No HIP type in here: the host twin needs no device.
//
// Input l[w][0..2] = log2 LIBD0/1/2 of window w and the switch penalties p01, p02, p12.  In quanta of 2^-16 bit:
//   emission   a NaN column, or a maximum that is not finite: e = (0, 0, 0) (the window says nothing).  Otherwise
//              d_s = l_s - max(l) (one fp64 subtraction), clamped below at -2^24, e_s = (int64) rint(d_s * 65536), ties to
//              even: the product is exact, so e_s is the same integer wherever it is formed
//   penalties  P_xy = llrint(log2(p_xy) * 65536) by the host's libm, clamped below at -2^40; 0 on the diagonal
//   recurrence score[0][s] = e_0[s], from[0][s] = s; score[i][s] = max_q(score[i-1][q] + pen[q][s]) + e_i[s], q = 0, 1, 2
//              with strict >: the lowest state wins a tie (argmax3 of hgpath.c)
//   traceback  from argmax3(score[n-1]), as hg_solve
// (max, +) over integers is exact and associative: the scores, hence the `from` entries, hence the path are the same
// integers for any blocking of the windows.  n_win <= 2^21 keeps |score| < 2^62 (a step moves a score by at most 2^40
// down -- its own state's emission -- and never up).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ibdg {

constexpr size_t STATES_MAX_WIN = (size_t)1 << 21;
constexpr double STATES_QUANTA = 65536.0;               // per bit
constexpr double STATES_D_MIN = -16777216.0;            // clamp of l_s - max(l), bits
constexpr int64_t STATES_PEN_MIN = -((int64_t)1 << 40); // clamp of a penalty, quanta

// P[0..2] = P_01, P_02, P_12; 1 if a p is NaN or outside (0, 1] (bad: its index 0..2)
int states_penalties(double p01, double p02, double p12, int64_t P[3], int *bad);

// the host twin (ibdg_log2_states_host): path [n_win] or NULL, score [n_win][3] or NULL, count[3]; err: room for a message
int log2_states_host(const double *tab, size_t n_win, double p01, double p02, double p12, uint8_t *path, int64_t *score,
                     uint64_t count[3], char *err, size_t err_len);

}  // namespace ibdg
