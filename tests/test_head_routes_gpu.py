"""The inference routes of a DynamicSegHead, pinned from outside: which kernels run, in which order, and with which bits.

  launch trace   every `_lib.call` of head(x), of two forward_shared calls on one memo and of two _layer1_fused calls on one memo,
                 for pointwise in ("f32", "split", "split3", False) x head_act in ("f32", "f16") x three grids, against the literal
                 lists of TRACES below.  The lists were RECORDED, not derived: this file's `record_traces` was run on commit 675b519
                 ("Heads, head_act="f16": layer 1's per-object half in one HIP launch"), before the routes were gathered into one
                 table per block, and its output pasted here.  The first call of a fresh head folds and packs its weights: the pack
                 launches are part of the lists.
  bits           the same matrix, torch.equal against a composition written out here from the per-kernel public ops alone
                 (constants from ops.fold_bn / ops.fold_pointwise; not through _folded, _pw or ops.conv1x1).  The composition
                 was run on that same commit as well and agreed with it in all 48 cases: a disagreement is the module's.
  ops.conv1x1    the typed wrapper's bits for each weight type; TypeError / ValueError for what it refuses.
  prepare_head_terms   count and stored terms equal to what forward_shared stores.

Grids: (10, 12) h*w = 120, every kernel eligible; (9, 12) 108, a multiple of 4 and not of 8: the f16 kernels ineligible, the MFMA
ones eligible; (9, 13) 117: the framework's 1x1.  cs = 100 shared channels, n in {1, 3} objects."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CS = 100
GRIDS = [(10, 12), (9, 12), (9, 13)]
POINTWISE = ["f32", "split", "split3", False]
HEAD_ACT = ["f32", "f16"]
NS = [1, 3]

# symbol names without their "manet_" prefix, in call order; "-" stands for "returned None without a launch".  One entry per
# (pointwise, head_act, (h, w)); the sequences do not depend on n (asserted for both).
#   "head"    head(x) on a fresh head
#   "shared"  forward_shared(shared, per_object, memo=m) twice with one m = {}
#   "layer1"  _layer1_fused(...) twice with one memo
TRACES = {
    ('f32', 'f32', (10, 12)):
    {'head': 'dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex conv1x1_f32 '
             'dwconv7x7_bn_relu_ex conv1x1_head_f32',
     'shared': ['dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex conv1x1_f32 conv1x1_add_f32 dwconv7x7_bn_relu_ex conv1x1_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex conv1x1_head_f32',
                'dwconv7x7_bn_relu_ex conv1x1_add_f32 dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex conv1x1_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_head_f32'],
     'layer1': ['dwconv7x7_bn_relu_ex conv1x1_f32 head_layer1_object_f32', 'head_layer1_object_f32']},
    ('f32', 'f32', (9, 12)):
    {'head': 'dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex conv1x1_f32 '
             'dwconv7x7_bn_relu_ex conv1x1_head_f32',
     'shared': ['dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex conv1x1_f32 conv1x1_add_f32 dwconv7x7_bn_relu_ex conv1x1_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex conv1x1_head_f32',
                'dwconv7x7_bn_relu_ex conv1x1_add_f32 dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex conv1x1_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_head_f32'],
     'layer1': ['dwconv7x7_bn_relu_ex conv1x1_f32 head_layer1_object_f32', 'head_layer1_object_f32']},
    ('f32', 'f32', (9, 13)):
    {'head': 'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
     'shared': ['dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
    ('f32', 'f16', (10, 12)):
    {'head': 'conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack dwconv7x7_bn_relu_f16 conv1x1_f16 '
             'dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16',
     'shared': ['conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack dwconv7x7_bn_relu_f16 conv1x1_f16 head_layer1_object_f16 '
                'dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16',
                'head_layer1_object_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 '
                'dwconv7x7_bn_relu_f16 conv1x1_f16'],
     'layer1': ['dwconv7x7_bn_relu_ex conv1x1_f32 head_layer1_object_f32', 'head_layer1_object_f32']},
    ('f32', 'f16', (9, 12)):
    {'head': 'conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_f32 conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_f32 '
             'conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_f32 conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_head_f32',
     'shared': ['conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex conv1x1_f32 '
                'conv1x1_add_f32 dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex '
                'conv1x1_head_f32',
                'dwconv7x7_bn_relu_ex conv1x1_add_f32 dwconv7x7_bn_relu_ex conv1x1_f32 dwconv7x7_bn_relu_ex conv1x1_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_head_f32'],
     'layer1': ['dwconv7x7_bn_relu_ex conv1x1_f32 head_layer1_object_f32', 'head_layer1_object_f32']},
    ('f32', 'f16', (9, 13)):
    {'head': 'conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_f16_pack '
             'dwconv7x7_bn_relu_ex conv1x1_f16_pack dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
     'shared': ['conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
    ('split', 'f32', (10, 12)):
    {'head': 'conv1x1_x3_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32 conv1x1_x3_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32 '
             'conv1x1_x3_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32 conv1x1_x3_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32',
     'shared': ['conv1x1_x3_pack conv1x1_x3_pack conv1x1_x3_pack dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex conv1x1_x3_f32 '
                'conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex '
                'conv1x1_x3_f32',
                'dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_x3_f32'],
     'layer1': ['-', '-']},
    ('split', 'f32', (9, 12)):
    {'head': 'conv1x1_x3_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32 conv1x1_x3_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32 '
             'conv1x1_x3_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32 conv1x1_x3_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32',
     'shared': ['conv1x1_x3_pack conv1x1_x3_pack conv1x1_x3_pack dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex conv1x1_x3_f32 '
                'conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex '
                'conv1x1_x3_f32',
                'dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_x3_f32'],
     'layer1': ['-', '-']},
    ('split', 'f32', (9, 13)):
    {'head': 'conv1x1_x3_pack dwconv7x7_bn_relu_ex conv1x1_x3_pack dwconv7x7_bn_relu_ex conv1x1_x3_pack dwconv7x7_bn_relu_ex '
             'conv1x1_x3_pack dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
     'shared': ['conv1x1_x3_pack conv1x1_x3_pack conv1x1_x3_pack dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
    ('split', 'f16', (10, 12)):
    {'head': 'conv1x1_x3_pack conv1x1_f16_pack conv1x1_x3_pack conv1x1_f16_pack conv1x1_x3_pack conv1x1_f16_pack '
             'conv1x1_x3_pack conv1x1_f16_pack dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 '
             'dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16',
     'shared': ['conv1x1_x3_pack conv1x1_x3_pack conv1x1_x3_pack conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack '
                'dwconv7x7_bn_relu_f16 conv1x1_f16 head_layer1_object_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 '
                'dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16',
                'head_layer1_object_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 '
                'dwconv7x7_bn_relu_f16 conv1x1_f16'],
     'layer1': ['-', '-']},
    ('split', 'f16', (9, 12)):
    {'head': 'conv1x1_x3_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32 conv1x1_x3_pack conv1x1_f16_pack '
             'dwconv7x7_bn_relu_ex conv1x1_x3_f32 conv1x1_x3_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32 '
             'conv1x1_x3_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_x3_f32',
     'shared': ['conv1x1_x3_pack conv1x1_x3_pack conv1x1_x3_pack conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack '
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex conv1x1_x3_f32 conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32',
                'dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 dwconv7x7_bn_relu_ex conv1x1_x3_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_x3_f32'],
     'layer1': ['-', '-']},
    ('split', 'f16', (9, 13)):
    {'head': 'conv1x1_x3_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_x3_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex '
             'conv1x1_x3_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_x3_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex '
             'relu_conv1x1_c1_f32',
     'shared': ['conv1x1_x3_pack conv1x1_x3_pack conv1x1_x3_pack conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack '
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
    ('split3', 'f32', (10, 12)):
    {'head': 'conv1x1_x6_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32 conv1x1_x6_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32 '
             'conv1x1_x6_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32 conv1x1_x6_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32',
     'shared': ['conv1x1_x6_pack conv1x1_x6_pack conv1x1_x6_pack dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex conv1x1_x6_f32 '
                'conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex '
                'conv1x1_x6_f32',
                'dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_x6_f32'],
     'layer1': ['-', '-']},
    ('split3', 'f32', (9, 12)):
    {'head': 'conv1x1_x6_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32 conv1x1_x6_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32 '
             'conv1x1_x6_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32 conv1x1_x6_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32',
     'shared': ['conv1x1_x6_pack conv1x1_x6_pack conv1x1_x6_pack dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex conv1x1_x6_f32 '
                'conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex '
                'conv1x1_x6_f32',
                'dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_x6_f32'],
     'layer1': ['-', '-']},
    ('split3', 'f32', (9, 13)):
    {'head': 'conv1x1_x6_pack dwconv7x7_bn_relu_ex conv1x1_x6_pack dwconv7x7_bn_relu_ex conv1x1_x6_pack dwconv7x7_bn_relu_ex '
             'conv1x1_x6_pack dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
     'shared': ['conv1x1_x6_pack conv1x1_x6_pack conv1x1_x6_pack dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
    ('split3', 'f16', (10, 12)):
    {'head': 'conv1x1_x6_pack conv1x1_f16_pack conv1x1_x6_pack conv1x1_f16_pack conv1x1_x6_pack conv1x1_f16_pack '
             'conv1x1_x6_pack conv1x1_f16_pack dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 '
             'dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16',
     'shared': ['conv1x1_x6_pack conv1x1_x6_pack conv1x1_x6_pack conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack '
                'dwconv7x7_bn_relu_f16 conv1x1_f16 head_layer1_object_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 '
                'dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16',
                'head_layer1_object_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 '
                'dwconv7x7_bn_relu_f16 conv1x1_f16'],
     'layer1': ['-', '-']},
    ('split3', 'f16', (9, 12)):
    {'head': 'conv1x1_x6_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32 conv1x1_x6_pack conv1x1_f16_pack '
             'dwconv7x7_bn_relu_ex conv1x1_x6_f32 conv1x1_x6_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32 '
             'conv1x1_x6_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_x6_f32',
     'shared': ['conv1x1_x6_pack conv1x1_x6_pack conv1x1_x6_pack conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack '
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex conv1x1_x6_f32 conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32',
                'dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 dwconv7x7_bn_relu_ex conv1x1_x6_f32 '
                'dwconv7x7_bn_relu_ex conv1x1_x6_f32'],
     'layer1': ['-', '-']},
    ('split3', 'f16', (9, 13)):
    {'head': 'conv1x1_x6_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_x6_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex '
             'conv1x1_x6_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_x6_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex '
             'relu_conv1x1_c1_f32',
     'shared': ['conv1x1_x6_pack conv1x1_x6_pack conv1x1_x6_pack conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack '
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
    (False, 'f32', (10, 12)):
    {'head': 'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
     'shared': ['dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
    (False, 'f32', (9, 12)):
    {'head': 'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
     'shared': ['dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
    (False, 'f32', (9, 13)):
    {'head': 'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
     'shared': ['dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
    (False, 'f16', (10, 12)):
    {'head': 'conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack dwconv7x7_bn_relu_f16 conv1x1_f16 '
             'dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16',
     'shared': ['conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack dwconv7x7_bn_relu_f16 conv1x1_f16 head_layer1_object_f16 '
                'dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16',
                'head_layer1_object_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 dwconv7x7_bn_relu_f16 conv1x1_f16 '
                'dwconv7x7_bn_relu_f16 conv1x1_f16'],
     'layer1': ['-', '-']},
    (False, 'f16', (9, 12)):
    {'head': 'conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_f16_pack '
             'dwconv7x7_bn_relu_ex conv1x1_f16_pack dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
     'shared': ['conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
    (False, 'f16', (9, 13)):
    {'head': 'conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_f16_pack dwconv7x7_bn_relu_ex conv1x1_f16_pack '
             'dwconv7x7_bn_relu_ex conv1x1_f16_pack dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
     'shared': ['conv1x1_f16_pack conv1x1_f16_pack conv1x1_f16_pack dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex relu_conv1x1_c1_f32',
                'dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex dwconv7x7_bn_relu_ex '
                'relu_conv1x1_c1_f32'],
     'layer1': ['-', '-']},
}


def _sym(fn):
    name = fn if isinstance(fn, str) else fn.__name__
    return name[len("manet_"):] if name.startswith("manet_") else name


class _Recorder:
    """stands in for _lib.call: notes the symbol, forwards"""

    def __init__(self, inner):
        self.inner, self.seq = inner, []

    def __call__(self, fn, *args):
        self.seq.append(_sym(fn))
        return self.inner(fn, *args)

    def take(self):
        out, self.seq = " ".join(self.seq), []
        return out


def make_env():
    """(ops, the IntVOS module, the state of a head whose BatchNorm statistics were randomised once from a fixed seed)"""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops
    from cvpr2020_manet_amd.networks import IntVOS as M
    torch.manual_seed(1234)
    with torch.no_grad():
        base = M.DynamicSegHead(in_dim=CS + 3, embed_dim=256).cuda().eval()
        for m in base.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 2.0); m.weight.normal_(1, 0.1); m.bias.normal_(0, 0.1)
    return ops, M, {k: v.clone() for k, v in base.state_dict().items()}


@pytest.fixture(scope="module")
def env():
    return make_env()


def make_head(env, pointwise, head_act):
    """a fresh head (nothing folded yet) with the shared parameters and statistics, stamped with the two modes"""
    ops, M, state = env
    head = M.DynamicSegHead(in_dim=CS + 3, embed_dim=256).cuda().eval()
    head.load_state_dict(state)
    for blk in head.modules():
        if isinstance(blk, M._split_separable_conv2d):
            object.__setattr__(blk, "_pw_mode", pointwise)
    return M.use_head_act(head, head_act)


_inputs = {}


def inputs(grid, n):
    """(shared [1, CS, h, w], per_object [n, 3, h, w], global map, local map [h, w, n], labels [h, w]): made once, never written"""
    if (grid, n) not in _inputs:
        from cvpr2020_manet_amd import ops
        h, w = grid
        g = torch.Generator().manual_seed(h * 100 + w * 10 + n)
        shared = (torch.relu(torch.randn(1, CS, h, w, generator=g)) * 0.3).cuda()
        gmap, lmap = torch.rand(h, w, n, generator=g).cuda(), torch.rand(h, w, n, generator=g).cuda()
        lab = torch.randint(0, n + 1, (h, w), generator=g, dtype=torch.int32).cuda()  # (one label value matches no object)
        _inputs[(grid, n)] = (shared, ops.head_inputs(gmap, lmap, lab, n, (h, w)), gmap, lmap, lab)
    return _inputs[(grid, n)]


def run_module(env, pointwise, head_act, grid, n, recorder=None):
    """the five module calls of one case on a fresh head: (outputs, traces)"""
    ops, M, _ = env
    h, w = grid
    shared, per, gmap, lmap, lab = inputs(grid, n)
    head = make_head(env, pointwise, head_act)
    take = recorder.take if recorder is not None else (lambda: "")
    take()  # (making the inputs may have launched ops.head_inputs: not the module's)
    out, tr = {}, {}
    with torch.no_grad():
        out["head"] = head(torch.cat((shared.repeat(n, 1, 1, 1), per), 1))
        tr["head"] = take()
        m = {}
        out["shared"], tr["shared"] = [], []
        for _ in range(2):
            out["shared"].append(head.forward_shared(shared, per, memo=m))
            tr["shared"].append(take())
        memo = {}
        out["layer1"], tr["layer1"] = [], []
        for _ in range(2):
            out["layer1"].append(M._layer1_fused(head.layer1, shared, gmap, lmap, lab, n, (h, w), memo=memo))
            tr["layer1"].append(take() or "-")
            assert recorder is None or (out["layer1"][-1] is None) == (tr["layer1"][-1] == "-")
    return out, tr


def record_traces(env, monkeypatch_setattr):
    """{case: traces} of the whole matrix (how TRACES was made); the sequences of n = 1 and n = 3 must agree"""
    from cvpr2020_manet_amd import _lib
    rec = _Recorder(_lib.call)
    monkeypatch_setattr(_lib, "call", rec)
    table = {}
    for pointwise in POINTWISE:
        for head_act in HEAD_ACT:
            for grid in GRIDS:
                per_n = [run_module(env, pointwise, head_act, grid, n, rec)[1] for n in NS]
                assert all(t == per_n[0] for t in per_n), (pointwise, head_act, grid)
                table[(pointwise, head_act, grid)] = per_n[0]
    return table


# ---- 1. the launch trace

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("head_act", HEAD_ACT)
@pytest.mark.parametrize("pointwise", POINTWISE, ids=str)
def test_launch_trace_is_the_recorded_one(env, monkeypatch, pointwise, head_act, grid, n):
    from cvpr2020_manet_amd import _lib
    rec = _Recorder(_lib.call)
    monkeypatch.setattr(_lib, "call", rec)
    _, got = run_module(env, pointwise, head_act, grid, n, rec)
    want = TRACES[(pointwise, head_act, grid)]
    for what in ("head", "shared", "layer1"):
        g, w_ = got[what], want[what]
        assert (g.split() if isinstance(g, str) else [s.split() for s in g]) == (
            w_.split() if isinstance(w_, str) else [s.split() for s in w_]), what


# ---- 2. the bits: the head composed by hand from the per-kernel ops

def _block_consts(ops, blk):
    scale1, shift1 = ops.fold_bn(blk.bn1)
    w2t, b2 = ops.fold_pointwise(blk.conv2, blk.bn2)
    return scale1, shift1, w2t, b2


def _conv_weight(w2t):
    """[Cin, 256] -> the framework's [256, Cin, 1, 1]"""
    return w2t.t().contiguous()[:, :, None, None]


def _one_by_one(ops, y, w2t, b2, route, relu=False, add=None, head=None):
    """a 1x1 stage on the typed public op of `route` ("f32" / "split" / "split3" / "f16"; None: the framework's convolution,
    a fused output layer behind it on ops.relu_conv1x1_c1)"""
    if route is None:
        assert add is None
        z = F.conv2d(y, _conv_weight(w2t), b2)
        if head is not None:
            return ops.relu_conv1x1_c1(z, head[0], head[1])
        return z.relu_() if relu else z
    kw = {"relu_out": relu, "add": add}
    if head is not None:
        kw.update(head_weight=head[0], head_bias=head[1])
    if route == "f32":
        return ops.conv1x1_mfma(y, w2t.contiguous(), b2, **kw)
    if route == "f16":
        return ops.conv1x1_f16(y, ops.HalfWeight(w2t), b2, **kw)
    return ops.conv1x1_split(y, ops.SplitWeight(w2t, pieces=3 if route == "split3" else 2), b2, **kw)


def _depthwise(ops, x, blk, scale1, shift1, f16, lo=None, hi=None):
    w1, b1 = blk.conv1.weight[lo:hi], blk.conv1.bias[lo:hi]
    fn = ops.dwconv7x7_bn_relu_f16 if f16 else ops.dwconv7x7_bn_relu
    return fn(x, w1, b1, scale=scale1[lo:hi], shift=shift1[lo:hi])


def _compose_tail(ops, head, x, route, f16):
    """layers 2-4 and the output layer; every block's ReLU in its own 1x1 stage, layer 4's fused with the output layer"""
    for blk in (head.layer2, head.layer3):
        scale1, shift1, w2t, b2 = _block_consts(ops, blk)
        x = _one_by_one(ops, _depthwise(ops, x, blk, scale1, shift1, f16), w2t, b2, route, relu=True)
    scale1, shift1, w2t, b2 = _block_consts(ops, head.layer4)
    return _one_by_one(ops, _depthwise(ops, x, head.layer4, scale1, shift1, f16), w2t, b2, route,
                       head=(head.conv.weight, head.conv.bias))


def compose(env, pointwise, head_act, grid, n):
    """what run_module's five calls must return, from the route rules alone:
      f16 applies when head_act == "f16", w is even and h*w a multiple of 8 (every stage on the f16 kernels, whatever `pointwise`);
      otherwise the 1x1 stages run on the kernel of `pointwise` when h*w is a multiple of 4, else on the framework's convolution;
      _layer1_fused exists for pointwise "f32" and h*w a multiple of 4 only, whatever head_act"""
    ops, M, _ = env
    h, w = grid
    shared, per, gmap, lmap, lab = inputs(grid, n)
    head = make_head(env, pointwise, head_act)
    f16 = head_act == "f16" and w % 2 == 0 and (h * w) % 8 == 0
    route = "f16" if f16 else (pointwise if pointwise and (h * w) % 4 == 0 else None)
    l1 = head.layer1
    out = {}
    with torch.no_grad():
        scale1, shift1, w2t, b2 = _block_consts(ops, l1)
        assert bool(torch.isfinite(w2t.half()).all())
        zero = torch.zeros_like(b2)
        # head(x): the concatenated input through layer 1 as a whole
        x = torch.cat((shared.repeat(n, 1, 1, 1), per), 1)
        x1 = _one_by_one(ops, _depthwise(ops, x, l1, scale1, shift1, f16), w2t, b2, route, relu=True)
        out["head"] = _compose_tail(ops, head, x1, route, f16)
        # forward_shared: the shared channels once, their term added in the per-object half's 1x1
        s1 = _depthwise(ops, shared, l1, scale1, shift1, f16, None, CS)
        if f16:
            term = ops.conv1x1_f16(s1, ops.HalfWeight(w2t[:CS]), zero, out_f32=True)
            x1 = ops.head_layer1_object_f16(per, l1.conv1.weight[CS:], l1.conv1.bias[CS:], scale1[CS:], shift1[CS:],
                                            ops.HalfWeight(w2t[CS:]), b2, term=term)
        else:
            p1 = _depthwise(ops, per, l1, scale1, shift1, False, CS, None)
            if route is None:
                x1 = F.conv2d(p1, _conv_weight(w2t[CS:]), b2)
                x1 += F.conv2d(s1, _conv_weight(w2t[:CS]), None)
                x1 = x1.relu_()
            else:
                term = _one_by_one(ops, s1, w2t[:CS], zero, route)
                x1 = _one_by_one(ops, p1, w2t[CS:], b2, route, relu=True, add=term)
        out["shared"] = _compose_tail(ops, head, x1, route, f16)
        # _layer1_fused: the exact-fp32 route's layer 1 straight from the maps
        out["layer1"] = None
        if pointwise == "f32" and (h * w) % 4 == 0:
            s1 = _depthwise(ops, shared, l1, scale1, shift1, False, None, CS)
            term = ops.conv1x1_mfma(s1, w2t[:CS].contiguous(), zero)
            out["layer1"] = ops.head_layer1_object(gmap, lmap, lab, n, (h, w), l1.conv1.weight[CS:], l1.conv1.bias[CS:],
                                                   scale1[CS:], shift1[CS:], w2t[CS:].contiguous(), b2, term, relu_out=True)
    return out


def compare_bits(env, pointwise, head_act, grid, n):
    got, _ = run_module(env, pointwise, head_act, grid, n)
    want = compose(env, pointwise, head_act, grid, n)
    assert tuple(got["head"].shape) == (n, 1) + grid and got["head"].dtype == torch.float32
    assert torch.equal(got["head"], want["head"])
    for y in got["shared"]:  # (the second call read the memo where the route keeps one)
        assert torch.equal(y, want["shared"])
    for y in got["layer1"]:
        assert (y is None) == (want["layer1"] is None)
        assert y is None or torch.equal(y, want["layer1"])


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("head_act", HEAD_ACT)
@pytest.mark.parametrize("pointwise", POINTWISE, ids=str)
def test_module_bits_equal_the_composition_by_hand(env, pointwise, head_act, grid, n):
    compare_bits(env, pointwise, head_act, grid, n)


# ---- 3. ops.conv1x1: the typed wrappers behind one front

def test_conv1x1_dispatches_on_the_weight_and_refuses_the_rest(env):
    ops = env[0]
    g = torch.Generator().manual_seed(3)
    h, w = 10, 12
    x = (torch.relu(torch.randn(2, 20, h, w, generator=g)) * 0.5).cuda()
    w2t, b2 = (torch.randn(20, 256, generator=g) * 0.1).cuda(), (torch.randn(256, generator=g) * 0.2).cuda()
    add = (torch.randn(1, 256, h, w, generator=g) * 0.3).cuda()
    hw_, hb_ = (torch.randn(1, 256, 1, 1, generator=g) * 0.1).cuda(), torch.full((1,), 0.05).cuda()
    forms = [{}, {"relu_out": True, "add": add}, {"head_weight": hw_, "head_bias": hb_}, {"head_weight": hw_}]
    cases = [(x, w2t, ops.conv1x1_mfma, ops.conv1x1_mfma_ok), (x, ops.SplitWeight(w2t), ops.conv1x1_split, ops.conv1x1_split_ok),
             (x, ops.SplitWeight(w2t, pieces=3), ops.conv1x1_split, ops.conv1x1_split_ok),
             (x.half(), ops.HalfWeight(w2t), ops.conv1x1_f16, ops.conv1x1_f16_ok)]
    for xin, weight, typed, typed_ok in cases:
        for kw in forms:
            got, want = ops.conv1x1(xin, weight, b2, **kw), typed(xin, weight, b2, **kw)
            assert got.dtype == want.dtype and torch.equal(got, want)
        for bad in (xin[:, :, :9, :], xin[:, :, :9, :9], xin[0]):  # h*w = 108 (% 4, not % 8), 81, and a 3-D tensor
            assert ops.conv1x1_ok(bad, weight) == typed_ok(bad, ops.PW_COUT)
        assert ops.conv1x1_ok(xin, weight) and typed_ok(xin, ops.PW_COUT) and not ops.conv1x1_ok(xin, weight, cout=128)
    half = ops.HalfWeight(w2t)
    got = ops.conv1x1(x.half(), half, b2, out_f32=True)
    assert got.dtype == torch.float32 and torch.equal(got, ops.conv1x1_f16(x.half(), half, b2, out_f32=True))
    for weight in (None, "f32", [w2t], w2t.cpu().numpy()):
        with pytest.raises(TypeError):
            ops.conv1x1(x, weight, b2)
        with pytest.raises(TypeError):
            ops.conv1x1_ok(x, weight)
    for weight in (w2t, ops.SplitWeight(w2t)):
        with pytest.raises(ValueError):
            ops.conv1x1(x, weight, b2, out_f32=True)
    with pytest.raises(ValueError):  # the exclusivity rule, once for all three
        ops.conv1x1(x, w2t, b2, add=add, head_weight=hw_)


# ---- 4. prepare_head_terms stores what forward_shared stores

@pytest.mark.parametrize("mode", ["f32", "f16", "split"])
def test_prepare_head_terms_stores_forward_shareds_terms(env, mode):
    from examples import propagate_clip as pc
    from cvpr2020_manet_amd.config import make_cfg
    ops, M, state = env
    dev = torch.device("cuda", 0)
    h, w = GRIDS[0]
    torch.manual_seed(0)
    cfg = make_cfg(["--TEST_MODE", "True"])
    kw = {"f32": {}, "f16": {"head_act": "f16"}, "split": {"pointwise": "split"}}[mode]
    model = M.IntVOS(cfg, pc.StandInEncoder(cfg.MODEL_ASPP_OUTDIM), **kw).to(dev).eval()
    head = model.dynamic_seghead
    head.load_state_dict(state)
    g = torch.Generator().manual_seed(9)
    emb = (torch.relu(torch.randn(3, CS, h, w, generator=g)) * 0.3).to(dev)
    per = inputs((h, w), 3)[1]
    with torch.no_grad():
        emb = model.prepare_clip(emb)
        count = model.prepare_head_terms(emb)
        if mode == "split":
            assert count == 0
            return
        assert count == 3 and model.prepare_head_terms(emb) == 3
        assert head._f16_ok(h, w, CS) == (mode == "f16")
        for i in range(3):
            stored = model._head_memo(emb[i], head)
            own = {}
            head.forward_shared(emb[i].float().unsqueeze(0), per, memo=own)
            assert stored["k"] is own["k"] and stored["stamp"] == own["stamp"]
            assert stored["term"].dtype == torch.float32 and tuple(stored["term"].shape) == (1, 256, h, w)
            assert torch.equal(stored["term"], own["term"])
