/* cagym_ig_credit.h -- the parameter block of the per-robot credit for the team reward: cagym_ig_credit (the call and its contract:
 * cagym.h; the rule in full: csrc/cagym_ig_credit.h).  cagym.h declares the type; a caller that fills one includes this header. */
#ifndef CAGYM_IG_CREDIT_H
#define CAGYM_IG_CREDIT_H
#include "cagym.h"

struct cagym_ig_credit_params {
    int32_t n_robots;   /* R, 1..8: rows per world; a row past the world's team is zero */
    uint32_t flags;     /* CAGYM_IG_EPISODE_FOLD | CAGYM_IG_OBSERVE_ONLY_RESTARTED, the values cagym_ig_observe was given */
    float detect_range; /* fp32: the detector emulation's range, rounded as cagym_ig_observe rounds its detect_range; finite, > 0 */
    double fov_rad;    /* sensor cone and range, as cagym_ig_observe's; finite, > 0 */
    double range;
};

#endif
