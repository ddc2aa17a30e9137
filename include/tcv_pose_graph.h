/* Batched 4-DoF pose-graph optimisation on the device: PoseGraph::optimize4DoF of the reference (pose_graph/src/pose_graph.cpp:403-579,
 * cost functors and angle parameterisation pose_graph.h:89-246) as one device batch of independent graphs.  It turns loop edges into
 * the drift-free poses that tcv_estimator_set_relo_frame (include/tcv_estimator_relo.h) takes as prev_relo_t / prev_relo_r, and into
 * the drift pair (r_drift, t_drift) the caller applies to the keyframes behind the last node.
 *
 * What finds a loop (descriptor database, PnP, the acceptance test) and the keyframe list stay with the caller.  There is no CPU path.
 *
 * Per graph: nodes 0 .. n_nodes-1 in keyframe order, parameters yaw (degrees, wrapped once like NormalizeAngle, :89-97) and t.  Node 0 and
 * every node with sequence == 0 are constant (:473-477).  Sequence edges to the up-to-four previous nodes of the same sequence (:480-495),
 * measured from the input poses on the device; loop edges (:499-514) with Huber loss.  Ceres' Levenberg-Marquardt loop with an exact
 * direct factorisation (band + dense border), FP64, fixed summation orders: the same bits from run to run and
 * whether a graph is solved alone or inside any batch.
 *
 * Limits (TCV_ERR_UNSUPPORTED before anything is launched): TCV_POSE_GRAPH_MAX_NODES nodes and TCV_POSE_GRAPH_MAX_LOOPS loop edges per
 * graph, TCV_POSE_GRAPH_MAX_BATCH graphs per call.  Valid C99 and C++14. */
#ifndef TCV_POSE_GRAPH_H
#define TCV_POSE_GRAPH_H
#include "tcv.h" /* the error codes */

#ifdef __cplusplus
extern "C" {
#endif

#define TCV_POSE_GRAPH_MAX_NODES 2048
#define TCV_POSE_GRAPH_MAX_LOOPS 256
#define TCV_POSE_GRAPH_MAX_BATCH 4096
#define TCV_POSE_GRAPH_MAX_TRACE 16

typedef struct tcv_pose_graph_desc {
    int n_nodes;
    const double *t;                 /* n_nodes x 3: VIO position                                                     */
    const double *q_xyzw;            /* n_nodes x 4: VIO orientation                                                  */
    const int *sequence;             /* n_nodes, NULL: all 1                                                          */
    int n_loops;
    const int *loop_cur, *loop_old;  /* local indices, loop_old < loop_cur                                            */
    const double *loop_relative_t;   /* n_loops x 3                                                                   */
    const double *loop_relative_yaw; /* n_loops, degrees                                                              */
} tcv_pose_graph_desc;

/* named after Ceres' Solver::Options and the constants of the reference; the defaults reproduce the reference */
typedef struct tcv_pose_graph_options {
    int max_num_iterations;             /* 5   (:437)                                                               */
    double huber_delta;                 /* 0.1 (:440); <= 0: no loss on the loop edges                              */
    double loop_weight;                 /* 1   (pose_graph.h:207)                                                   */
    double loop_yaw_divisor;            /* 10  (pose_graph.h:231)                                                   */
    double function_tolerance;          /* 1e-6                                                                     */
    double gradient_tolerance;          /* 1e-10                                                                    */
    double parameter_tolerance;         /* 1e-8                                                                     */
    double initial_trust_region_radius; /* 1e4                                                                      */
    double min_relative_decrease;       /* 1e-3                                                                     */
} tcv_pose_graph_options;
void tcv_pose_graph_options_default(tcv_pose_graph_options *o);

typedef struct tcv_pose_graph_summary {
    int iterations;  /* records: iteration 0 + accepted + rejected + invalid steps (may exceed TCV_POSE_GRAPH_MAX_TRACE)        */
    int termination; /* as tcv_solver_summary::termination: 0 NO_CONVERGENCE 1 gradient 2 parameter 3 function 4 radius 5 FAILURE */
    int num_free_nodes, num_edges; /* of the reduced problem: edges between two constant nodes only add to the fixed cost      */
    double initial_cost, final_cost; /* fixed cost included                                                                   */
    /* the first TCV_POSE_GRAPH_MAX_TRACE records; cost excludes the fixed cost, as the minimiser sees it */
    double cost[TCV_POSE_GRAPH_MAX_TRACE], cost_candidate[TCV_POSE_GRAPH_MAX_TRACE], rho[TCV_POSE_GRAPH_MAX_TRACE], radius[TCV_POSE_GRAPH_MAX_TRACE];
    int step[TCV_POSE_GRAPH_MAX_TRACE]; /* 1 accepted (and iteration 0), 0 rejected (and the record of a tolerance stop), -1 invalid */
    double yaw_drift, r_drift[9], t_drift[3]; /* :549-557, r_drift row-major                                                  */
} tcv_pose_graph_summary;

/* All n graphs as ONE device batch: one upload, one kernel sequence on `hip_stream` (NULL, a hipStream_t or TCV_STREAM_THREAD), one
 * download; returns when the results are on the host.  t_out[g]: n_nodes x 3, R_out[g]: n_nodes x 9 row-major (either array, or an entry,
 * may be NULL).  options NULL: the defaults.  A graph whose factorisation keeps failing reports termination 5 in its own summary and
 * comes back with the last accepted poses (never NaN); it does not fail the call.
 * TCV_ERR_INVALID (before the device is touched): NULL arrays, n_nodes < 1, indices out of range, loop_old >= loop_cur, non-finite input. */
int tcv_pose_graphs_optimize(int n, const tcv_pose_graph_desc *descs, const tcv_pose_graph_options *options, double *const *t_out,
                             double *const *R_out, tcv_pose_graph_summary *summaries, void *hip_stream);

/* Residual and Jacobians of n independent edges on the device (the counterpart of tcv_eval_projection_factors).  kind[k]: 0 sequence
 * edge, 1 loop edge (weight, yaw divisor and Huber corrector of `options` applied, as the solver sees them).  Per edge: yaw_i, t_i (older
 * node), yaw_j, t_j, measurement [relative_t 3 | relative_yaw | pitch_i | roll_i].  Out: residual 4, jacobian 32 = d r / d (yaw_i, t_i)
 * 4 x 4 row-major | d r / d (yaw_j, t_j) 4 x 4, cost (rho / 2). */
int tcv_pose_graph_eval_edges(int n, const int *kind, const double *yaw_i, const double *t_i, const double *yaw_j, const double *t_j,
                              const double *measurement, const tcv_pose_graph_options *options, double *residual, double *jacobian, double *cost);

/* Host only: the elimination order of one graph.  out[8] = { free nodes, band nodes, border nodes, edges of the reduced problem, edges of
 * the fixed cost, scalar half-bandwidth of the band, scratch bytes on the device, 0 }; position (n_nodes ints, may be NULL): -1 constant,
 * 0 .. band-1 band, band .. free-1 border. */
int tcv_pose_graph_plan_stats(const tcv_pose_graph_desc *desc, long long *out, int *position);

/* The calling thread's last tcv_pose_graphs_optimize: out[4] = host packing, upload, kernel, download in milliseconds (the three
 * device figures from events on the call's stream). */
int tcv_pose_graph_last_timing(double *out);

#ifdef __cplusplus
}
#endif
#endif
