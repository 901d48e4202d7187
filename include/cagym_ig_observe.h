/* cagym_ig_observe.h -- the parameter block of the fused learner observation (the call and its contract: cagym.h).
 * cagym.h declares the type; a caller that fills one includes this header. */
#ifndef CAGYM_IG_OBSERVE_H
#define CAGYM_IG_OBSERVE_H
#include "cagym.h"

struct cagym_ig_observe_params {
    int32_t n_robots;    /* 1..8: the IG robots of every scenario of the pool */
    int32_t window;      /* G: cells per side of a robot's belief window, even, 4..64 */
    int32_t rotate;      /* 1: window rows run along the robot's heading; 0: along +x */
    uint32_t flags;      /* CAGYM_IG_EPISODE_FOLD | CAGYM_IG_OBSERVE_ONLY_RESTARTED */
    double detect_range; /* the detector emulation's range, as the argument of that name of the robot-inputs call */
    double fov_rad;      /* sensor cone and range of the belief update, as the update call's arguments */
    double range;
};

#endif
