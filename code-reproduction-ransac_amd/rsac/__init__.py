"""rsac -- MI355X-native RANSAC engine (PnP camera pose + homography).

Drop-in for the RANSAC hot path of Mendel0408/Code-Reproduction-RANSAC, whose
scripts call cv2.solvePnPRansac (main_v1.py:497) and cv2.findHomography
(main_v1.py:312).  The compute runs in hand-written HIP kernels for gfx950
(librsac.so, built from ../csrc) reached through a ctypes C ABI
(include/rsac.h).  See DESIGN.md.
"""
from ._lib import Context, RsacError, context, lib  # noqa: F401
from . import dem  # noqa: F401
from .api import (LocationResult, OrientationResult, RansacInfo, Scan, compute_reprojection_error,  # noqa: F401
                  epnp_minimal, epnp_pose, estimate_camera_orientation, evaluate_range, fundamental_ransac, homography_fit,
                  homography_ransac, homography_ransac_batched, hypotheses, intrinsics_grid, local_opt,
                  location_search, pnp_ransac, pnp_ransac_batched, pnp_ransac_first_round, pnp_ransac_batched_rows, pnp_ransac_batched_flat, pose_mask, refine_pose,
                  project_points, refine_pose_device, reprojection_errors, rodrigues, score_poses, undistort_points,
                  update_num_iters, winner, msac_shift, pose_cost, homography_lmeds, homography_lmeds_batched,
                  hom_median, lmeds_sigma, lmeds_num_iters, LmedsScan, homography_costs, homography_cost,
                  fundamental_lmeds, fundamental_costs, fundamental_errors, fundamental_cost, fm_median,
                  fundamental_fit, fundamental_local_opt, homography_fit_batched, homography_local_opt, pnp_lmeds, pnp_lmeds_batched, pnp_medians, pnp_median,
                  fundamental_ransac_batched, fundamental_lmeds_batched, fundamental_fit_batched,
                  fundamental_local_opt_batched, fundamental_minimal7, cubic_real_roots,
                  essential_ransac, essential_ransac_batched, essential_minimal5, poly_real_roots,
                  essential_from_fundamental, recover_pose, essential_refine, essential_refine_batched,
                  essential_local_opt, essential_local_opt_batched, essential_to_fundamental, EssentialFitInfo)

__all__ = ["pnp_ransac", "pnp_ransac_batched", "pnp_ransac_batched_flat", "homography_ransac", "homography_ransac_batched", "score_poses",
           "evaluate_range", "hypotheses", "pose_mask", "refine_pose", "homography_fit", "rodrigues", "update_num_iters",
           "location_search", "LocationResult", "local_opt", "dem", "epnp_minimal", "epnp_pose", "fundamental_ransac", "winner", "Scan", "Context", "context", "RsacError", "RansacInfo", "lib",
           "estimate_camera_orientation", "OrientationResult", "intrinsics_grid", "reprojection_errors",
           "compute_reprojection_error", "refine_pose_device", "pnp_ransac_first_round",
           "pnp_ransac_batched_rows", "undistort_points", "project_points", "msac_shift", "pose_cost",
           "homography_lmeds", "homography_lmeds_batched", "hom_median", "lmeds_sigma", "lmeds_num_iters", "LmedsScan",
           "homography_costs", "homography_cost", "fundamental_lmeds", "fundamental_costs", "fundamental_errors",
           "fundamental_cost", "fm_median", "fundamental_fit", "fundamental_local_opt", "homography_fit_batched", "homography_local_opt", "pnp_lmeds", "pnp_lmeds_batched",
           "pnp_medians", "pnp_median", "fundamental_ransac_batched", "fundamental_lmeds_batched",
           "fundamental_fit_batched", "fundamental_local_opt_batched", "fundamental_minimal7", "cubic_real_roots",
           "essential_ransac", "essential_ransac_batched", "essential_minimal5", "poly_real_roots",
           "essential_from_fundamental", "recover_pose", "essential_refine", "essential_refine_batched",
           "essential_local_opt", "essential_local_opt_batched", "essential_to_fundamental", "EssentialFitInfo"]
