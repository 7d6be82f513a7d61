"""Golden vectors for ``control.sample_inputs_face``, produced BY THE REFERENCE'S OWN FUNCTIONS.  Their modules import
diffusers / cv2 / gradio at import time, so the FunctionDef nodes are taken from the source files in place (ast) and executed
in a namespace that only holds torch -- no reference text enters the repo:
  Keypoint/mofa_keypoint.py: sample_inputs_face (:36-63)
  Keypoint/utils/utils.py:   sample_optical_flow (:81-103), get_sparse_flow (:106-119)
The fixture holds tensors only: first_frame [3,40,56], 5 frames of 68 landmarks as fp32 and as fp16 (what the reference
passes), and the six outputs of each run.  The dense 384 x 384 outputs are stored compactly: the sparse flows and masks as
sparse tensors, first_frame_384 -- a nearest resize of a first frame whose values are multiples of 1/16 -- as uint8 (x 16).
    python tests/golden/make_golden_control_face.py"""
import ast
import os

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_golden_control_face.pt")


def take(path, names, ns):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            node.decorator_list = []
            exec(compile(ast.Module([node], []), path, "exec"), ns)
    missing = [n for n in names if n not in ns]
    assert not missing, missing


ns = {"torch": torch, "F": F}
take("/root/reference/MOFA-Video-Keypoint/utils/utils.py", ["sample_optical_flow", "get_sparse_flow"], ns)
take("/root/reference/MOFA-Video-Keypoint/mofa_keypoint.py", ["sample_inputs_face"], ns)

g = torch.Generator().manual_seed(11)
first_frame = torch.randint(0, 17, (3, 40, 56), generator=g).float() / 16
lm = torch.rand(5, 68, 2, generator=g) * torch.tensor([60.0, 44.0]) - 2.0           # (x, y) pixels, a little beyond 56 x 40
lm[0, 3], lm[0, 7] = lm[0, 12], lm[0, 12] + 0.01                                    # three landmarks on one pixel
G = {"first_frame": first_frame, "landmarks_fp32": lm, "landmarks_fp16": lm.half()}
for tag in ("fp32", "fp16"):
    image, flow, mask, ff384, flow384, mask384 = ns["sample_inputs_face"](first_frame, G["landmarks_" + tag].clone())
    x16 = (ff384 * 16).round().to(torch.uint8)
    assert torch.equal(x16.float() / 16, ff384)
    G[tag] = dict(controlnet_image=image, sparse_optical_flow=flow.to_sparse(), mask=mask.to_sparse(), first_frame_384_x16=x16,
                  sparse_optical_flow_384=flow384.to_sparse(), mask_384=mask384.to_sparse())
assert torch.equal(G["fp32"]["first_frame_384_x16"], G["fp16"]["first_frame_384_x16"])
del G["fp16"]["first_frame_384_x16"]                                                 # the same image: stored once
torch.save(G, OUT)
print({k: (list(v) if isinstance(v, dict) else tuple(v.shape)) for k, v in G.items()}, os.path.getsize(OUT))
