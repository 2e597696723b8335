/* pqp_search_params.h — the parameter struct of pqp_speed_search (include/pqp.h, which includes this file and states what the fields mean
 * in the definition; the numbers in front of each comment are pqp_search_default_params' values).  A header of its own, read beside
 * pqp.h by the Python binding's reader (path_optimizer_2_amd/pqp_header.py) and held against the compiler's layout by
 * tests/test_speed_search.py. */
#ifndef PQP_SEARCH_PARAMS_H_
#define PQP_SEARCH_PARAMS_H_
#include <stdint.h>

typedef struct pqp_search_params {
    double dt;                /* 1.0   s, finite, > 0: the time between layers; layer k is at time k dt */
    double ds;                /* 0.5   m, finite, > 0: the distance between stations; station j is at arc length j ds */
    double w_slow;            /* 1.0   finite, >= 0: price per layer and per cell of step below what the envelope admits (qref) */
    double w_accel;           /* 1.0   finite, >= 0: price per squared change of the step, in cells */
    double margin;            /* 0.0   m, finite, >= 0: pqp_agents_check's margin */
    int32_t stations;         /* 128   S >= 1 */
    int32_t q_max;            /* 20    Q, the largest step in cells per layer, 0 <= Q <= 63 */
    int32_t q_up;             /* 3     the step may grow by at most this per layer, >= 0 */
    int32_t q_down;           /* 6     and shrink by at most this, >= 0 */
} pqp_search_params;

#endif /* PQP_SEARCH_PARAMS_H_ */
