"""Host restatements for the device-resident scene tests (tests/test_scene_cpu.py, tests/test_scene_gpu.py)."""
import numpy as np

FLIP = np.array([1.0, -1.0, -1.0])


def proj_f64(K, poses):
    """proj[k] = K . diag(1,-1,-1) . pose[k] as pnrf_scene_select_fwd forms it: fp32 operands, products and the left-to-right three-term sums as
    explicit element-wise float64 operations, one rounding to fp32.  K [3,3], poses [n,3,4] -> [n,3,4] float32."""
    K = np.asarray(K, dtype=np.float32).astype(np.float64)
    P = np.asarray(poses, dtype=np.float32).astype(np.float64)[:, :3, :4] * FLIP[None, :, None]          # sign flips: exact
    out = np.empty((P.shape[0], 3, 4), np.float64)
    for r in range(3):
        for c in range(4):
            out[:, r, c] = (K[r, 0] * P[:, 0, c] + K[r, 1] * P[:, 1, c]) + K[r, 2] * P[:, 2, c]
    return out.astype(np.float32)


def proj_exact_and_bound(K, poses):
    """float64 K @ F @ pose and the element-wise bound 4 . 2^-24 . (|K| . |F . pose|): gamma_3 = 3 u / (1 - 3 u) of an fp32 three-term dot product
    (u = 2^-24) plus half an ulp (<= u |result|) for a final rounding — what any evaluation of the product in fp32 or better stays within."""
    K = np.asarray(K, dtype=np.float32).astype(np.float64)
    P = np.asarray(poses, dtype=np.float32).astype(np.float64)[:, :3, :4] * FLIP[None, :, None]
    exact = np.einsum('rj,njc->nrc', K, P)
    bound = 4.0 * 2.0 ** -24 * np.einsum('rj,njc->nrc', np.abs(K), np.abs(P))
    return exact, bound
