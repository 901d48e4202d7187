/* cagym_ig_episode_log.h -- the zero-copy views of the information-gathering team's episode log (the calls and their contract:
 * cagym.h).  cagym.h declares the type; a caller that reads the views includes this header. */
#ifndef CAGYM_IG_EPISODE_LOG_H
#define CAGYM_IG_EPISODE_LOG_H
#include "cagym.h"

struct cagym_ig_episode_log_ptrs {
    const uint32_t* key;                 /* ring [L] ... */
    const int32_t *world, *episode;
    const int64_t* slice;
    const int32_t* steps;
    const double* ret;
    const int32_t *n_targets, *n_found;
    const int32_t* found_at;             /* [L,M] */
    const double *entropy, *residual_mi;
    const int32_t* n_touched;
    const int32_t *steps_run, *found_run; /* running [N], [N,M] */
    const int32_t* cursor;
    const uint64_t* head;
    const int32_t* desync;
    int32_t capacity;
};

#endif
