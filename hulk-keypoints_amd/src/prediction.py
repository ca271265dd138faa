"""MI355X-native restatement of src/prediction.py (Prediction, :8-66).

predict() is the reference's (:16-24).  keypoints() is the fused decode the
north star asks for: the argmax of plot() (:46, np.unravel_index(h.argmax()),
first max wins) computed on the GPU inside the upsample kernel, so no
[B,K,H,W] heatmap has to cross PCIe.  plot() keeps the reference's output
(JET overlays in a 2-column grid written to preds/out%04d.png) using numpy/PIL
when OpenCV is absent — cv2.normalize / addWeighted / circle(r=4, filled)
restated; the JET table is analytic, so pixel parity with cv2 is unpinned;
expectation() keeps the reference's (dead, :45) math and soft_argmax() is its
fixed form on the GPU (hkp_soft_argmax).
"""
import os

import numpy as np
import torch


class Prediction:
    def __init__(self, model, num_keypoints, img_height, img_width, use_cuda):
        self.model = model
        self.num_keypoints = num_keypoints
        self.img_height = img_height
        self.img_width = img_width
        self.use_cuda = use_cuda

    @staticmethod
    def _batch(imgs):
        if len(imgs.shape) == 4:
            return imgs.view(-1, imgs.shape[1], imgs.shape[2], imgs.shape[3])
        if len(imgs.shape) == 3:
            return imgs.view(-1, imgs.shape[0], imgs.shape[1], imgs.shape[2])
        return imgs

    def predict(self, imgs):
        # img: torch.Tensor(3, height, width) or (B, 3, height, width)
        return self.model.forward(self._batch(imgs))

    def keypoints(self, imgs):
        """int32 [B,K,2] (y, x) argmax per heatmap, computed on the GPU."""
        return self.model.predict_keypoints(self._batch(imgs))

    def peaks(self, imgs, **kw):
        """(float32 [B,K,P,3] (x, y, score), int32 [B,K] counts): the up to P =
        max_peaks local maxima per heatmap with sub-pixel positions and scores,
        computed on the GPU from the low-res logits — (x, y), not the (y, x) of
        keypoints().  kw: max_peaks, radius, threshold (KeypointsGauss.predict_peaks)."""
        return self.model.predict_peaks(self._batch(imgs), **kw)

    def groups(self, imgs, classes, **kw):
        """(peaks, counts, group int32 [B,K,P], tag float32 [B,K,P]): peaks() and, for the
        class indices `classes`, the cable each peak belongs to, grouped on the GPU by the
        model's tag maps (a model trained with tags).  kw: max_peaks, radius, threshold,
        max_dist (KeypointsGauss.predict_groups); no tta."""
        return self.model.predict_groups(self._batch(imgs), classes, **kw)

    def evaluate(self, imgs, labels, metrics, **kw):
        """peaks(), matched on the GPU to `labels` ([B,K,M,3] (u, v, flag) or [B,K,2]) and
        added into `metrics` (hkp.metrics.KeypointMetrics); kw as for peaks().  Returns
        what peaks() returns (KeypointsGauss.evaluate)."""
        return self.model.evaluate(self._batch(imgs), labels, metrics, **kw)

    def softmax(self, x):
        e_x = np.exp(x - np.max(x))
        return e_x / e_x.sum()

    def expectation(self, d):
        """prediction.py:31-38, vectorised (same values, including its index mapping)."""
        width, height = d.T.shape
        d = d.T.ravel()
        d_norm = self.softmax(d)
        i = np.arange(width * height)
        return [int(np.dot(d_norm, i % width)), int(np.dot(d_norm, i // width))]

    @staticmethod
    def _jet(u8):
        x = u8.astype(np.float32) / np.float32(255.0)
        r = np.clip(np.float32(1.5) - np.abs(np.float32(4) * x - np.float32(3)), 0, 1)
        g = np.clip(np.float32(1.5) - np.abs(np.float32(4) * x - np.float32(2)), 0, 1)
        b = np.clip(np.float32(1.5) - np.abs(np.float32(4) * x - np.float32(1)), 0, 1)
        return (np.stack([b, g, r], -1) * np.float32(255)).astype(np.uint8)  # BGR like cv2.COLORMAP_JET

    @staticmethod
    def disc_halfwidths(r=4):
        """Row half-widths of cv2.circle(img, c, r, color, -1) (LINE_8: OpenCV's
        midpoint Circle rasteriser, imgproc/drawing.cpp) for rows |dy| = 0..r."""
        hw = [-1] * (r + 1)
        err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
        while dx >= dy:
            hw[dy] = max(hw[dy], dx)
            if dx <= r:
                hw[dx] = max(hw[dx], dy)
            dy += 1
            err += plus
            plus += 2
            mask = -1 if err > 0 else 0
            err -= minus & mask
            dx += mask
            minus -= mask & 2
        return hw

    @staticmethod
    def _normalize_u8(h):
        """cv2.normalize(h, None, 0, 255, NORM_MINMAX) (double scale / shift into a
        float32 image), then .astype(np.uint8) (prediction.py:48)."""
        mn, mx = float(h.min()), float(h.max())
        sc = 255.0 / (mx - mn) if mx - mn > np.finfo(np.float64).eps else 0.0
        v = (h.astype(np.float64) * sc + (0.0 - mn * sc)).astype(np.float32)
        return np.clip(v, 0, 255).astype(np.uint8)

    def soft_argmax(self, heatmaps, beta=1.0):
        """float32 [B,K,2] (x, y) on the GPU: Prediction.expectation (prediction.py:31-38)
        with its axis mix-up fixed — softmax(beta * h)-weighted mean position."""
        from hkp import ops
        return ops.soft_argmax(heatmaps.contiguous(), beta)

    def expectation_fixed(self, d, beta=1.0):
        """numpy restatement of soft_argmax for one [H,W] plane: (x, y) floats."""
        d = np.asarray(d, dtype=np.float64)
        e = np.exp(beta * d - np.max(beta * d))
        p = e / e.sum()
        ys, xs = np.mgrid[0:d.shape[0], 0:d.shape[1]]
        return float((p * xs).sum()), float((p * ys).sum())

    def overlays(self, imgs_u8, heatmaps=None, keypoints=None):
        """Prediction.plot's picture for a whole batch on the GPU:
        uint8 [B, H*K/2, 2W, 3] BGR on the device, bit-identical to plot()'s numpy
        restatement.  imgs_u8: [B,H,W,3] uint8 (BGR); heatmaps / keypoints default to
        one fused forward of the model on imgs_u8."""
        from hkp import ops
        imgs_u8 = imgs_u8.to("cuda").contiguous()
        if heatmaps is None or keypoints is None:
            heatmaps, keypoints = self.model.heatmaps_and_keypoints(imgs_u8)
        return ops.heat_overlay(heatmaps.contiguous(), imgs_u8, keypoints.to(torch.int32).contiguous())

    def plot(self, img, heatmap, image_id=0, cls=None, classes=None, keypoints=None, out_dir="preds"):
        print("Running inferences on image: %d" % image_id)
        overlays = []
        for i in range(self.num_keypoints):
            h = heatmap[0][i]
            if keypoints is not None:
                pred_y, pred_x = (int(v) for v in keypoints[0][i])
            else:
                pred_y, pred_x = np.unravel_index(h.argmax(), h.shape)
            vis = self._jet(self._normalize_u8(h))
            blend = np.float32(0.65) * img.astype(np.float32) + np.float32(0.35) * vis.astype(np.float32)
            overlay = np.clip(np.rint(blend), 0, 255).astype(np.uint8)         # cv2.addWeighted
            hw = self.disc_halfwidths(4)                                        # cv2.circle(.., 4, (0,0,0), -1)
            for dy in range(-4, 5):
                y = pred_y + dy
                if 0 <= y < overlay.shape[0]:
                    x0, x1 = max(0, pred_x - hw[abs(dy)]), min(overlay.shape[1], pred_x + hw[abs(dy)] + 1)
                    overlay[y, x0:x1] = 0
            overlays.append(overlay)
        half = self.num_keypoints // 2
        col1 = np.concatenate(overlays[:half], 0) if half else None
        col2 = np.concatenate(overlays[half:], 0)
        result = col2 if col1 is None else np.concatenate([col1, col2], 1)
        os.makedirs(out_dir, exist_ok=True)
        from PIL import Image
        Image.fromarray(result[:, :, ::-1]).save(os.path.join(out_dir, "out%04d.png" % image_id))
        return result
