"""numpy restatement of article_separation/plot_net_output.py:196-241 and of its blend (:57-93), for the tests of the
segmentation net evaluation.  tests/test_seg_eval_host.py holds it to the reference's own compute_accuracy, apply_mask and
plot_image_with_net_output through tests/golden/seg_eval_golden.npz."""
import numpy as np

MASK_COLOR = (255, 50, 50)


def score(prob, gts=None, mask_threshold=False):
    """prob float32 [H,W,C], gts uint8 [C,H,W] or None -> dict of exact integers and the masks, as the reference computes them"""
    out_img = np.asarray(prob, np.float32)[None]
    C = out_img.shape[-1]
    res = {"unsure": int(np.sum((0 < out_img) & (out_img < 1))), "size": int(out_img.size)}       # :198-199
    if mask_threshold:
        out_img = np.array((out_img > 0.6), np.int32)                                              # :201-202
    values = np.argmax(out_img, axis=3)                                                             # :216
    one_hot = np.zeros_like(out_img)
    np.put_along_axis(one_hot, values[..., None], 1, axis=3)                                        # :221-225
    res["class_count"] = [int(np.sum(values == c)) for c in range(C)]                               # :226
    res["masks"] = np.stack([np.uint8(out_img[0, :, :, cl] * 255) for cl in range(C)])              # :232-234
    res["one_hot"] = one_hot[0]
    if gts is not None:
        gts = np.asarray(gts, np.uint8)
        res["equal"] = [int(np.sum(one_hot[0, :, :, cl] == gts[cl] / 255)) for cl in range(C)]      # :117,241
        res["accuracy_terms"] = [np.sum(one_hot[0, :, :, cl] == gts[cl] / 255) / gts[cl].size for cl in range(C)]
        hyp, pos = [values[0] == cl for cl in range(C)], [gts[cl] == 255 for cl in range(C)]
        res["tp"] = [int(np.sum(hyp[cl] & pos[cl])) for cl in range(C)]
        res["fp"] = [int(np.sum(hyp[cl] & ~pos[cl])) for cl in range(C)]
        res["fn"] = [int(np.sum(~hyp[cl] & pos[cl])) for cl in range(C)]
    return res


def accuracy(res):
    """:230,241,279"""
    acc = 0
    for term in res["accuracy_terms"]:
        acc += term
    return acc / len(res["accuracy_terms"])


def blend(scan, mask, color=MASK_COLOR, alpha=0.5):
    """apply_mask (:57-70) on scan.astype(uint32) as :245 calls it, then the uint8 of :253"""
    image = np.asarray(scan).astype(np.uint32)
    for c in range(3):
        image[:, :, c] = np.where(mask == 255, image[:, :, c] * (1 - alpha) + alpha * color[c], image[:, :, c])
    return np.uint8(image)


def page_lines(res, full_count, with_accuracy=True):
    """the reference's printed lines of a page (:198-199,227-228,281-282)"""
    lines = ["Percentage of Pixels where the net is not 100% sure:  " + str(res["unsure"] / res["size"])]
    for i, n in enumerate(res["class_count"]):
        lines.append(f"Percentage of pixels in class_{i}: {n / full_count}")
    lines.append("Accuracy =  " + str(accuracy(res) if with_accuracy else 0.0))
    lines.append("+++++++++++++++++++++++")
    return lines


def save_images(scan_bgr, masks, gts, plot_with_gt, plot_with_img):
    """:231-253: what is written per class (arrays as the file holds them, read back as gray or R, G, B)"""
    img = scan_bgr
    out = []
    for cl in range(len(masks)):
        o = masks[cl]
        if plot_with_img:
            img = img[:, :, ::-1]                                   # :244, once per class
            o = blend(img, masks[cl])
        if plot_with_gt:
            g = gts[cl]
            if plot_with_img:
                img = blend(img, g)                                 # :249 in place: the scan keeps the ground truth blend
                g = img
            o = np.concatenate((o, g), axis=1)
        out.append(np.ascontiguousarray(o))
    return out
