"""The kernel families the parity suites run every case on (not a test module): how a handle is
pinned to one of them, and the per-problem assertion they share.  Used by
test_gpu_config_fields.py (fp64) and test_gpu_fp32_parity.py (fp32)."""
import numpy as np

# family -> (layout id, options, what iterate_kernel must name): as test_gpu_parity.py and
# tools/parity_campaign.py pin them
BICYCLE_FAMILIES = {
    "wave": (0, {"group_lanes": 64}, "k_iterate"),
    "group": (0, {"group_lanes": 8, "speculate": 0, "group_workspace": 0}, "k_group_iterate"),
    "group-ws": (0, {"group_lanes": 8, "speculate": 0, "group_workspace": 1},
                 "k_group_iterate (workspace form)"),
    "spec": (0, {"group_lanes": 8, "speculate": 1}, "k_group_spec"),
    "row16": (0, {"group_lanes": 16, "speculate": 0}, "k_group_iterate (sixteen lanes)"),
    "lane": (1, {}, ("k_lane_iterate", "k_lane_iterate_pair")),
    "tiled": (2, {}, ("k_lane_iterate", "k_lane_iterate_pair")),
}
QUAD_FAMILIES = {
    "wave": (0, {"group_lanes": 64}, "k_iterate"),
    "quad16": (0, {"group_lanes": 16}, "k_quad_iterate"),
    "lane": (1, {}, "k_lane_iterate_rows"),
    "tiled": (2, {}, "k_lane_iterate_rows"),
}


def families(plant):
    return QUAD_FAMILIES if plant == "quad12" else BICYCLE_FAMILIES


def family_solver(cfg, plant, fam, B):
    """A handle of a copy of cfg on the family's layout, pinned to the family; iterate_kernel (and on
    quad12's lane layouts solve_kernel) must name it, so a silent fallback cannot pass for coverage."""
    from ilqr_iterative_tasks_amd import BatchedILQR
    lid, options, name = families(plant)[fam]
    cfg = cfg.copy()
    cfg.layout = lid
    solver = BatchedILQR(cfg)
    for key, val in options.items():
        solver.set_option(key, val)
    solver.ensure_workspace(B)
    got = solver.iterate_kernel(B)
    assert got in name if isinstance(name, tuple) else got == name, (fam, got)
    if name == "k_lane_iterate_rows":
        assert solver.solve_kernel(B) == name
    return solver, cfg


def assert_within(err, limit, what):
    over = err > limit
    worst = int(np.argmax(err / limit)) if len(err) else 0
    assert not over.any(), (f"{what}: {int(over.sum())} problems over their bound, worst "
                            f"{float((err / limit).max()):.2f} x (error {float(err[worst]):.3e}, "
                            f"bound {float(limit[worst]):.3e}, entry {worst})")
