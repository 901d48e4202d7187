/* cagym_ig_context.h -- the parameter block of the learner's context window (the call and its contract: cagym.h).
 * cagym.h declares the type; a caller that fills one includes this header. */
#ifndef CAGYM_IG_CONTEXT_H
#define CAGYM_IG_CONTEXT_H
#include "cagym.h"

struct cagym_ig_context_params {
    int32_t n_robots; /* 1..8: the IG robots of every scenario of the pool */
    int32_t window;   /* G: cells per side, even, 4..64 - the belief window's, for the two images to share their sample points */
    int32_t rotate;   /* 1: window rows run along the robot's heading; 0: along +x - the belief window's */
    uint32_t flags;   /* CAGYM_IG_CONTEXT_ONLY_MASKED */
    double clear_max; /* metres at which the clearance channel saturates at 1, finite, > 0 */
};

#endif
