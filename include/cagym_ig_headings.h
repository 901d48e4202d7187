/* cagym_ig_headings.h -- the parameter block of the heading-resolved view gains: cagym_ig_view_gain_headings (the call and its
 * contract: cagym.h).  cagym.h declares the type; a caller that fills one includes this header.  The call validates the whole
 * block. */
#ifndef CAGYM_IG_HEADINGS_H
#define CAGYM_IG_HEADINGS_H
#include "cagym.h"

struct cagym_ig_heading_params {
    int32_t n_points;    /* P >= 0: viewpoints per world of points_xy [N,P,2] (ignored with points_xy NULL: 3600) */
    int32_t n_headings;  /* H, 1..16: the headings scored at every viewpoint */
    uint32_t flags;      /* none defined: 0 (four bytes of padding follow) */
    double radius;       /* metres; a viewpoint is valid when EDF(point) > radius + 0.1, the planners' feasibility test; finite, > 0 */
    double range;        /* metres, the sensing range of cagym_ig_visible_cells; finite, > 0 */
    double fov;          /* radians, the full opening angle of the sensor cone, as cagym_ig_visible_cells takes it; finite, > 0 */
    double headings[16]; /* radians, the caller's; the first H must be finite */
};

#endif
