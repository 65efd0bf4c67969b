"""Numpy restatements for the mesh-evaluation tests (csrc/nnsearch.hip, utils/mesh_eval.py): the brute-force nearest
neighbour search, the voxel down-sample, face normals and areas, and the two metric dictionaries.

fp64 throughout, except the voxel coordinate, which repeats the kernel's separately rounded fp32 operations."""
import numpy as np


def nearest(reference, query, chunk=512, second=False):
    """For every query the index (smallest on ties) and distance of the closest reference point, in fp64, by brute
    force over chunks of queries.  ``second``: also the distance to the second-nearest point (inf for one point)."""
    ref = np.asarray(reference, np.float64)
    qry = np.asarray(query, np.float64)
    nq = len(qry)
    idx = np.zeros(nq, np.int64)
    d1 = np.zeros(nq, np.float64)
    d2 = np.full(nq, np.inf, np.float64)
    chunk = max(1, min(chunk, int(4e7 // max(1, len(ref)))))
    for a in range(0, nq, chunk):
        q = qry[a:a + chunk]
        sq = np.zeros((len(q), len(ref)), np.float64)
        for d in range(3):
            diff = q[:, d, None] - ref[None, :, d]
            sq += diff * diff
        i = np.argmin(sq, axis=1)                          # first occurrence of the minimum: the smallest index
        rows = np.arange(len(q))
        idx[a:a + chunk] = i
        d1[a:a + chunk] = np.sqrt(sq[rows, i])
        if second and len(ref) > 1:
            sq[rows, i] = np.inf
            d2[a:a + chunk] = np.sqrt(sq.min(axis=1))
    return (d1, idx, d2) if second else (d1, idx)


def voxel_down_sample(points, voxel_size):
    """fp32 points [N,3] -> fp32 [M,3]: voxel = floor((p - (min_bound - v/2)) / v) with every operation rounded in
    fp32; per occupied voxel the fp64 sum of its points in ascending index over their count, rounded once to fp32;
    voxels in ascending (ix, iy, iz)."""
    p = np.ascontiguousarray(points, np.float32)
    v = np.float32(voxel_size)
    o = (p.min(axis=0) - v * np.float32(0.5)).astype(np.float32)
    c = np.floor(((p - o).astype(np.float32) / v).astype(np.float32)).astype(np.int64)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    order = np.argsort(key, kind='stable')
    sk = key[order]
    start = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    end = np.concatenate([start[1:], [len(p)]])
    out = np.empty((len(start), 3), np.float32)
    p64 = p.astype(np.float64)
    single = end - start == 1
    out[single] = p[order[start[single]]]
    for s in np.flatnonzero(~single):
        acc = np.zeros(3, np.float64)
        for e in order[start[s]:end[s]]:                    # ascending original index (stable sort)
            acc = acc + p64[e]
        out[s] = (acc / np.float64(end[s] - start[s])).astype(np.float32)
    return out


def face_cross(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


def face_areas(vertices, faces):
    return 0.5 * np.linalg.norm(face_cross(vertices, faces), axis=1)


def face_normals(vertices, faces):
    c = face_cross(vertices, faces)
    n = np.linalg.norm(c, axis=1, keepdims=True)
    return np.where(n > 0, c / np.where(n > 0, n, 1.0), 0.0)


def fscore(p, r):
    return 2.0 * p * r / (p + r) if p + r > 0 else 0.0


def scannet_metrics(pred, gt, threshold=0.05):
    """evaluate() of the ScanNet protocol on two (already down-sampled) clouds."""
    dist1, _ = nearest(pred, gt)                            # target -> predicted
    dist2, _ = nearest(gt, pred)                            # predicted -> target
    prec = float(np.mean(dist2 < threshold))
    recal = float(np.mean(dist1 < threshold))
    return {'Acc': float(np.mean(dist2)), 'Comp': float(np.mean(dist1)), 'Prec': prec, 'Recal': recal,
            'F-score': fscore(prec, recal)}


def replica_metrics(rec_points, rec_normals, gt_points, gt_normals, dist_th=0.05):
    """calc_3d_metric of the Replica protocol on given surface samples and their face normals."""
    d_acc, i_gt = nearest(gt_points, rec_points)            # rec -> gt
    d_comp, i_rec = nearest(rec_points, gt_points)          # gt -> rec
    rn, gn = np.asarray(rec_normals, np.float64), np.asarray(gt_normals, np.float64)
    n_acc = float(np.abs((rn * gn[i_gt]).sum(1)).mean())
    n_comp = float(np.abs((gn * rn[i_rec]).sum(1)).mean())
    acc, comp = float(d_acc.mean()), float(d_comp.mean())
    prec, ratio = float(np.mean(d_acc < dist_th)), float(np.mean(d_comp < dist_th))
    return {'accuracy': acc * 100, 'completion': comp * 100, 'precision': prec * 100, 'completion_ratio': ratio * 100,
            'fscore': fscore(prec, ratio) * 100, 'chamfer': (acc * 100 + comp * 100) / 2,
            'normal_acc': n_acc * 100, 'normal_comp': n_comp * 100, 'normal_avg': (n_acc + n_comp) * 0.5 * 100}
