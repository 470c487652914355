"""Inputs, yardstick and mutants shared by tests/test_eval_u8_cpu.py and tests/test_eval_u8_gpu.py (the eval-mode head,
svit_head_eval, and its NumPy restatement evaluate.head_eval_host).

The bar.  Metric: max |out - out64| per output tensor (class probabilities, boxes, contact), out64 = head_eval_host in
float64.  Yardstick: the same metric for SViTHead in fp32 eval mode -- the stock ATen head, existing code -- on the same
inputs (and, in the GPU test, the same device).  A kernel passes inside 4 x yardstick, floored at 2^-24 (half an ulp of a
probability near 1: the yardstick can be exactly 0 on a saturated output); the 4 x covers another summation order and
another exp.  Four mutants of the restatement, evaluated in fp32, must each land at least 10 x above that bar on at
least one output tensor -- a bar they passed would not notice the bug."""
import numpy as np
import torch

FLOOR = 2.0 ** -24
MUTANTS = ("no_bias", "cls_from_row_1", "softmax_without_max", "contact_from_objects_1_2")
HOT, COLD = 120.0, -800.0


def make_case(B, N, C, T, O, n_cls, seed, hot=True):
    """tokens f32 [B,N,C] ~ N(0,1) (a LayerNorm's output), weights ~ N(0, 1/C) so that logits are O(1), biases ~ N(0,1).
    hot: the cls row of clip B-1 is a multiple of class 0's weight row, so that its logit 0 is +120 (and the others
    O(10)); the first object row of clip 0 likewise along contact weight 0.  And the cold rows, logits of -800, whose
    exp(-z) overflows fp32 and fp64 alike (a sigmoid written 1 / (1 + exp(-z)) with a fast reciprocal gives NaN there):
    the cls row of clip 1 along the last class, object 2 of clip 1's first frame along the objectness weight, object 3
    along box weight 0 (needs B >= 2, O >= 4)."""
    g = np.random.default_rng(seed)
    f = np.float32
    tokens = g.standard_normal((B, N, C)).astype(f)
    params = []
    for rows in (n_cls, 4, 1, 5):
        params.append(((g.standard_normal((rows, C)) / np.sqrt(C)).astype(f), g.standard_normal(rows).astype(f)))
    if hot:
        w = params[0][0][0].astype(np.float64)
        tokens[B - 1, 0] = (w * (HOT - float(params[0][1][0])) / float(w @ w)).astype(f)
        w = params[3][0][0].astype(np.float64)
        tokens[0, N - T * O] = (w * (HOT - float(params[3][1][0])) / float(w @ w)).astype(f)
        for row, (wm, bm), k in ((0, params[0], n_cls - 1), (N - T * O + 2, params[2], 0), (N - T * O + 3, params[1], 0)):
            w = wm[k].astype(np.float64)
            tokens[1, row] = (w * (COLD - float(bm[k])) / float(w @ w)).astype(f)
    return tokens, params


def cold_outputs(outs, n_cls, act):
    """the outputs the cold rows drive to sigmoid(-800): class n_cls-1 of clip 1 (act 1 only), objectness of object 2
    and box 0 of object 3 of clip 1's first frame"""
    probs, boxes = outs[0], outs[1]
    return ([float(probs[1, n_cls - 1])] if act == 1 else []) + [float(boxes[1, 0, 2, 0]), float(boxes[1, 0, 3, 1])]


def errors(got, want64):
    """max |got - want64| per output tensor (probabilities, boxes, contact); a NaN or an infinity counts as inf"""
    out = []
    for g, w in zip(got[:3], want64[:3]):
        g = np.asarray(g.detach().cpu().numpy() if torch.is_tensor(g) else g, dtype=np.float64).reshape(w.shape)
        d = np.abs(g - w)
        out.append(float("inf") if not np.isfinite(d).all() else float(d.max()))
    return out


def bar(yardstick):
    return [max(4.0 * y, FLOOR) for y in yardstick]


def aten_head(tokens, params, T, O, act, device="cpu", dtype=torch.float32):
    """SViTHead.forward in eval mode (stock ATen ops) on these tokens and parameters -> (probs, boxes, contact)"""
    from svit_amd import config
    from svit_amd.model import SViTHead
    B, N, C = tokens.shape
    head = SViTHead(config.ssv2_cfg(num_frames=4, crop=64), C, params[0][0].shape[0],
                    act_func="softmax" if act == 0 else "sigmoid")
    with torch.no_grad():
        for (w, b), (pw, pb) in zip(params, head.param_pairs()):
            pw.copy_(torch.from_numpy(w))
            pb.copy_(torch.from_numpy(b))
    head = head.to(device=device, dtype=dtype).eval()
    x = torch.from_numpy(tokens).to(device=device, dtype=dtype)
    with torch.no_grad():
        feat = torch.cat((x[:, :1], x[:, N - T * O:]), dim=1)
        probs, extra = head(feat, T=T)
    return probs, extra["pred_bboxes"], extra["pred_contact_state"], extra["obj_desc"]


def mutant(name, tokens, params, T, O, act):
    """the restatement with one bug, in fp32 -> (probs, boxes, contact)"""
    from svit_amd.evaluate import head_eval_host
    f = np.float32
    B, N, C = tokens.shape
    if name == "no_bias":
        return head_eval_host(tokens, [(w, np.zeros_like(b)) for w, b in params], T, O, act, dtype=f)[:3]
    if name == "cls_from_row_1":
        t = tokens.copy()
        t[:, 0] = tokens[:, 1]
        return head_eval_host(t, params, T, O, act, dtype=f)[:3]
    if name == "contact_from_objects_1_2":
        t = tokens.copy()
        obj = tokens[:, N - T * O:].reshape(B, T, O, C)
        t[:, N - T * O:] = np.roll(obj, -1, axis=2).reshape(B, T * O, C)
        good = head_eval_host(tokens, params, T, O, act, dtype=f)
        return good[0], good[1], head_eval_host(t, params, T, O, act, dtype=f)[2]
    if name == "softmax_without_max":
        good = head_eval_host(tokens, params, T, O, act, dtype=f)

        def soft(z):
            with np.errstate(over="ignore", invalid="ignore"):
                e = np.exp(z.astype(f))
                return (e / e.sum(axis=-1, keepdims=True)).astype(f)
        (wp, bp), _, _, (wc, bc) = params
        probs = soft(tokens[:, 0] @ wp.T + bp) if act == 0 else good[0]
        xobj = tokens[:, N - T * O:].reshape(B, T, O, C)
        return probs, good[1], soft(xobj[:, :, :2] @ wc.T + bc)
    raise ValueError(name)


def caught(name, tokens, params, T, O, act, want64, bars):
    """the largest ratio error / bar over the output tensors of a mutant"""
    err = errors(mutant(name, tokens, params, T, O, act), want64)
    return max(e / b for e, b in zip(err, bars))
