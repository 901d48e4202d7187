/* cagym_ig_assign.h -- the parameter block of the team's goal assignment: cagym_ig_assign_goals (the call and its contract:
 * cagym.h; the rule in full: csrc/cagym_ig_assign.h).  cagym.h declares the type; a caller that fills one includes this header.
 * The call validates the whole block. */
#ifndef CAGYM_IG_ASSIGN_H
#define CAGYM_IG_ASSIGN_H
#include "cagym.h"

#define CAGYM_IG_ASSIGN_SLOT 0 /* the masked robots choose in slot order */
#define CAGYM_IG_ASSIGN_BEST 1 /* every round the best (robot, candidate) left among the masked robots */

struct cagym_ig_assign_params {
    int32_t n_robots; /* R, 1..8: the robots per world */
    int32_t k;        /* 1..16: candidates per robot */
    int32_t mode;     /* CAGYM_IG_ASSIGN_SLOT or CAGYM_IG_ASSIGN_BEST */
    uint32_t flags;   /* none defined: 0 */
    double radius;    /* metres; a candidate is valid when EDF(point) > radius + 0.1, cagym_ig_view_gain's rule; finite, > 0 */
    double range;     /* metres, the sensing range of both kinds of cell set; finite, > 0 */
    double d0;        /* metres added to the distance in the utility marginal / (distance + d0); finite, > 0 */
    double fov;       /* radians, the cone's full opening angle for a candidate with a finite heading - the fov the caller hands
                         cagym_ig_visible_cells; finite, > 0 (a call without headings validates it too) */
};

#endif
