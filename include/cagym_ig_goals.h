/* cagym_ig_goals.h -- the parameter block of the learner's goal actions: cagym_ig_geodesic, cagym_ig_goal_actions and
 * cagym_ig_goal_status (the calls and their contract: cagym.h).  cagym.h declares the type; a caller that fills one includes this
 * header.  Every call validates the whole block, whichever fields it uses. */
#ifndef CAGYM_IG_GOALS_H
#define CAGYM_IG_GOALS_H
#include "cagym.h"

struct cagym_ig_goal_params {
    int32_t n_robots; /* 1..8: the IG robots of every scenario of the pool */
    int32_t window;   /* G: cells per side of the belief window a goal cell (a, b) refers to, even, 4..64 */
    int32_t rotate;   /* 1: window rows run along the robot's heading; 0: along +x - the belief window's */
    uint32_t flags;   /* none defined: 0 */
    double radius;    /* metres; a cell is free when EDF(centre) > radius + 0.1, the planners' feasibility test; finite, > 0 */
    double v_max;     /* m/s the controller drives at once it is aligned; finite, > 0 */
    double w_max;     /* rad/s, the turn-rate clamp; finite, > 0 */
    double align_tol; /* rad: the robot moves only when the heading error left after this step's turn is at most this; finite, > 0 */
    double goal_tol;  /* metres from the goal point at which goal_reached is set and the robot stops; finite, > 0 */
    double dt;        /* seconds per step, the env's; finite, > 0 */
};

#endif
