/* cagym_ig_route.h -- the parameter block of the route gains: cagym_ig_route_gains (the call and its contract: cagym.h; the rule in
 * full: csrc/cagym_ig_route.h).  cagym.h declares the type; a caller that fills one includes this header.  The call validates the
 * whole block. */
#ifndef CAGYM_IG_ROUTE_H
#define CAGYM_IG_ROUTE_H
#include "cagym.h"

#define CAGYM_IG_ROUTE_MAX_WAYPOINTS 16 /* way-points per candidate: the second-last extent of way_cells, the last of way_dir */

struct cagym_ig_route_params {
    int32_t n_robots; /* R, 1..8: the robots per world */
    int32_t k;        /* 1..16: candidates per robot */
    int32_t stride;   /* >= 1: path cells between two way-points */
    uint32_t flags;   /* none defined: 0 */
    double radius;    /* metres; the candidate's own set is empty unless EDF(cell centre) > radius + 0.1, cagym_ig_view_gain's rule;
                         finite, > 0 */
    double range;     /* metres, the sensing range of every cell set; finite, > 0 */
    double fov;       /* radians, the cone's full opening angle at the way-points and at a candidate with a finite heading - the fov
                         the caller hands cagym_ig_visible_cells; finite, > 0 */
    double d0;        /* metres added to the distance in the utility total_gain / (field[cell] + d0); finite, > 0 */
};

#endif
