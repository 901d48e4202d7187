/* cagym_ig_viewpoints.h -- the parameter block of the view gains and goal proposals: cagym_ig_view_gain and cagym_ig_propose_goals
 * (the calls and their contract: cagym.h).  cagym.h declares the type; a caller that fills one includes this header.  Both calls
 * validate the whole block, whichever fields they use. */
#ifndef CAGYM_IG_VIEWPOINTS_H
#define CAGYM_IG_VIEWPOINTS_H
#include "cagym.h"

struct cagym_ig_view_params {
    int32_t n_points; /* P >= 0: viewpoints per world of cagym_ig_view_gain's points_xy [N,P,2] (ignored with points_xy NULL: 3600) */
    int32_t n_robots; /* R, 1..8: the robots per world of cagym_ig_propose_goals' mask, field and outputs */
    int32_t k;        /* 1..16: proposals per robot */
    uint32_t flags;   /* none defined: 0 */
    double radius;    /* metres; a viewpoint is valid when EDF(point) > radius + 0.1, the planners' feasibility test; finite, > 0 */
    double range;     /* metres, the sensing range: a cell is in range when |centre - point|^2 < range^2; finite, > 0 */
    double min_sep;   /* metres between the centres of two proposals of one robot; finite, > 0 */
    double d0;        /* metres added to the geodesic distance in the utility gain / (distance + d0); finite, > 0 */
};

#endif
