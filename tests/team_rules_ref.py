"""The reference's three team rules restated in Python for the tests (ref src/Agent.cpp:567-585, 1123-1156,
1280-1330), line by line in the reference's order.  A status is a dict with the fields of AgentStatus, or None where
the robot's status is absent; p is any object with the fields of dcora_team_params."""
import numpy as np

INITIALIZED = 2


def ready_to_terminate(p, robust, weight_update_count, success, relative_change, accepted, rejected, total):
    ready = True
    if not success:
        ready = False
    tol = p.rel_change_tol
    if robust and weight_update_count == 0:
        tol = 5
    if relative_change > tol:
        ready = False
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (np.float64(accepted) + np.float64(rejected)) / np.float64(total)
    if ratio < p.robust_opt_min_convergence_ratio:
        ready = False
    return ready


def should_terminate(p, robust, iteration_number, weight_update_count, statuses, active=None):
    if iteration_number >= p.max_num_iters:
        return True
    if robust and weight_update_count < p.robust_opt_num_weight_updates:
        return False
    for q, st in enumerate(statuses):
        if active is not None and not active[q]:
            continue
        if st is None:
            return False
        if st["state"] != INITIALIZED:
            return False
        if not st["ready_to_terminate"]:
            return False
    return True


def should_update_weights(p, robust, weight_update_count, inner_iter, latest_weight_update_iteration, statuses,
                          active=None):
    if not robust:
        return False
    if weight_update_count >= p.robust_opt_num_weight_updates:
        return False
    if inner_iter >= p.robust_opt_inner_iters:
        return True
    for q, st in enumerate(statuses):
        if active is not None and not active[q]:
            continue
        if st is None:
            return False
        if st["iteration_number"] < latest_weight_update_iteration:
            return False
        if st["state"] != INITIALIZED:
            return False
        if not st["ready_to_terminate"]:
            return False
    return True
