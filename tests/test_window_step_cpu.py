"""gbp_ba_window_step without a GPU: the ctypes structs against include/gbp_ba.h, the id translation of the host composition
(tests/window_host.py) on a hand-made graph, and what the lists of the GPU tests promise (tests/test_window_step_gpu.py)."""
import ctypes as ct
import os
import re

import numpy as np

from conftest import REPO
from window_host import WindowMaps, base_case, check_case, compose, filter_batch, four_calls, new_factor_ids_of_extend


def _header_struct(name):
    """field names of `typedef struct <name> { ... }` in include/gbp_ba.h, in order, with 'p' for pointers and 'i' for int32_t"""
    text = open(os.path.join(REPO, 'include', 'gbp_ba.h')).read()
    body = re.search(r'typedef struct %s \{(.*?)\} %s_t;' % (name, name), text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(','):                             # every pointer declarator of these structs carries its own '*'
            fields.append((re.search(r'(\w+)\s*$', part).group(1), 'p' if '*' in part else 'i'))
    return fields


def test_window_structs_match_the_header():
    from gbp_amd import _capi
    for cls, name in ((_capi.Window, 'gbp_ba_window'), (_capi.WindowMaps, 'gbp_ba_window_maps')):
        fields = _header_struct(name)
        assert [f for f, _ in fields] == [f for f, _ in cls._fields_], name
        off = 0
        for (fname, kind), (_, ctype) in zip(fields, cls._fields_):
            size = 4 if kind == 'i' else 8
            assert ct.sizeof(ctype) == size, fname
            off = (off + size - 1) // size * size
            assert getattr(cls, fname).offset == off, fname
            off += size
        assert ct.sizeof(cls) == (off + 7) // 8 * 8
    assert ct.sizeof(_capi.Window) == 16 + 4 * 8 and ct.sizeof(_capi.WindowMaps) == 6 * 8
    assert 'gbp_ba_window_step' in _capi.SIGNATURES and 'gbp_ba_rebuild_count' in _capi.SIGNATURES


class _ListGraph:
    """A graph as three id lists with the four calls' renumbering rules and nothing else: enough to follow ids through four_calls."""

    def __init__(self, C, L, cam, lmk):
        self.C, self.L, self.cam, self.lmk = C, L, list(cam), list(lmk)
        self.tag = list(range(len(self.cam)))                    # which original observation each factor is (batch: 100 + entry)

    def sizes(self):
        return self.C, self.L, len(self.cam)

    def extend(self, b):
        n_old = len(self.cam)
        cam, lmk = self.cam + list(b['cam_idx']), self.lmk + list(b['lmk_idx'])
        tag = self.tag + [100 + j for j in range(len(b['cam_idx']))]
        order = np.argsort(cam, kind='stable')
        self.cam, self.lmk, self.tag = [cam[k] for k in order], [lmk[k] for k in order], [tag[k] for k in order]
        self.C, self.L = self.C + len(b['cam_means']), self.L + len(b['lmk_means'])
        pos = np.empty(order.size, np.int64)
        pos[order] = np.arange(order.size)
        return pos[:n_old].astype(np.int32)

    def _shrink(self, keep_f, drop_c=()):
        from retire_host import renumbering
        cam, lmk = np.array(self.cam), np.array(self.lmk)
        keep_c = np.isin(np.arange(self.C), cam[keep_f]) & ~np.isin(np.arange(self.C), list(drop_c))
        keep_l = np.isin(np.arange(self.L), lmk[keep_f])
        cm, lm, fm = renumbering(keep_c), renumbering(keep_l), renumbering(keep_f)
        self.cam, self.lmk = list(cm[cam[keep_f]]), list(lm[lmk[keep_f]])
        self.tag = [t for t, k in zip(self.tag, keep_f) if k]
        self.C, self.L = int(keep_c.sum()), int(keep_l.sum())
        return cm, lm, fm

    def cull(self, ids):
        return self._shrink(~np.isin(np.arange(len(self.cam)), ids))

    def retire(self, ids):
        return self._shrink(~np.isin(self.cam, ids), drop_c=ids)

    def retire_landmarks(self, ids, fold):
        return self._shrink(~np.isin(self.lmk, ids))


def test_id_translation_on_a_three_camera_graph():
    """3 cameras, 4 landmarks, 7 observations; the batch brings camera 3, landmark 4 and three observations, one of them a late one of
    camera 1.  Cull old factor 3, retire camera 0, let go of landmark 2: every list in the numbering from before the step."""
    g = _ListGraph(3, 4, cam=[0, 0, 1, 1, 1, 2, 2], lmk=[0, 1, 0, 1, 2, 2, 3])
    batch = dict(cam_means=np.zeros((1, 6)), lmk_means=np.zeros((1, 3)), meas=np.zeros((3, 2)),
                 cam_idx=np.array([3, 1, 3], np.int32), lmk_idx=np.array([1, 3, 4], np.int32))
    m = four_calls(g, batch, cull=[3], retire=[0], lmks=[2])
    # after extend: cam 0:[f0 f1] 1:[f2 f3 f4 b1] 2:[f5 f6] 3:[b0 b2]; f3 culled; camera 0 retired (f0, f1); landmark 2 listed (f4, f5)
    assert g.tag == [2, 101, 6, 100, 102]
    np.testing.assert_array_equal(m.factor_map, [-1, -1, 0, -1, -1, -1, 2])
    np.testing.assert_array_equal(m.new_factor_ids, [3, 1, 4])
    np.testing.assert_array_equal(m.cam_map, [-1, 0, 1])
    np.testing.assert_array_equal(m.new_cam_ids, [2])
    np.testing.assert_array_equal(m.lmk_map, [0, 1, -1, 2])       # landmark 1 lost f1 and f3 but the new keyframe sees it
    np.testing.assert_array_equal(m.new_lmk_ids, [3])
    assert g.cam == [0, 0, 1, 2, 2] and g.lmk == [0, 2, 2, 1, 3]
    np.testing.assert_array_equal(compose([2, -1, 0], [5, 6, 7]), [7, -1, 5])
    np.testing.assert_array_equal(new_factor_ids_of_extend([0, 1, 2, 3, 4, 6, 7], [3, 1, 3]), [8, 5, 9])
    fb = filter_batch(batch, [1], [4])
    np.testing.assert_array_equal(fb['cam_idx'], [3])
    assert isinstance(m, WindowMaps)


def test_the_lists_of_the_gpu_tests_have_their_properties():
    c = base_case()
    goes = check_case(c)
    assert c.base.n_cams == 16 and 0 < goes.sum() < c.base.n_factors
    assert len(c.batch['cam_means']) == 2 and (c.batch['cam_idx'] < 16).sum() > 50


def test_the_shrinking_calls_live_in_the_window_unit():
    """gbp_ba_cull, gbp_ba_retire and gbp_ba_retire_landmarks are fronts of the window step's engine (gbp_capi_window.hip): the library
    is built from files that exist, still exports all four, and each refuses a null handle before it touches a device."""
    from gbp_amd import build, _capi
    for name in build.SOURCES + build.HEADERS:
        assert os.path.isfile(os.path.join(build.CSRC, name)), name
    assert len(set(build.SOURCES)) == len(build.SOURCES) and 'gbp_capi_window.hip' in build.SOURCES
    unit = open(os.path.join(build.CSRC, 'gbp_capi_window.hip')).read()
    build.build()
    lib = _capi.load()
    ids = np.zeros(1, np.int32)
    for name, args in (('gbp_ba_cull', (1, _capi.iptr(ids), None, None, None)), ('gbp_ba_retire', (1, _capi.iptr(ids), None, None, None)),
                       ('gbp_ba_retire_landmarks', (1, _capi.iptr(ids), _capi.RETIRE_FOLD, None, None, None)),
                       ('gbp_ba_window_step', (ct.byref(_capi.Window()), None))):
        assert re.search(r'^int %s\(' % name, unit, re.M), name
        assert getattr(lib, name)(None, *args) == -1, name
        assert b'null handle' in lib.gbp_last_error(), name
