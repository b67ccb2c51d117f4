"""CPU: the persistent solve's counter block (flamed-tts_amd/csrc/persist.hpp arrive_image, exported host-side as
flamed_persist_ctr_layout; no GPU).  Every (group, shard) arrival word lies on a 128-B line of its own, no group word
of any form shares a line with a GroupNorm counter or the error word, the launch's reset prologue covers the whole
block, each workgroup signals a word that its group's wait polls, and the per-word targets of the sharded and the
one-word image count the same 32 arrivals per hand-off for every hand-off number a solve can reach.
"""
import ctypes

import pytest

from flamed import _native as nat

LINE = 32  # ints per 128-B line
GROUPS, SLOTS = 8, 32
ONE_WORD = 4194304
DEFAULT = 885322


def _layout(opt, g, s, L=1):
    img = (ctypes.c_int * 7)()
    gn, err, n, rs = (ctypes.c_int() for _ in range(4))
    assert nat.lib().flamed_persist_ctr_layout(opt, g, s, L, img, ctypes.byref(gn), ctypes.byref(err), ctypes.byref(n),
                                               ctypes.byref(rs)) == 0
    keys = ("sig", "base", "stride", "n", "abase", "an", "mul")
    return dict(zip(keys, img)), gn.value, err.value, n.value, rs.value


def _polled(im, all_groups):
    b, n = (im["abase"], im["an"]) if all_groups else (im["base"], im["n"])
    return [b + k * im["stride"] for k in range(n)]


def test_shard_words_on_lines_of_their_own():
    words = set()
    for g in range(GROUPS):
        for s in range(SLOTS):
            im = _layout(DEFAULT, g, s)[0]
            assert im["mul"] == 8 and im["n"] == 4
            assert im["sig"] == _polled(im, False)[s // 8]  # shard k takes slots 8 k .. 8 k + 7
            words.add(im["sig"])
    assert len(words) == GROUPS * 4
    assert all(w % LINE == 0 for w in words) and len({w // LINE for w in words}) == GROUPS * 4
    assert sorted(_polled(_layout(DEFAULT, 3, 5)[0], True)) == sorted(words)


@pytest.mark.parametrize("opt", [DEFAULT, DEFAULT | ONE_WORD])
def test_block_is_covered_and_lines_are_not_shared(opt):
    _, _, err, ctr_ints, reset_ints = _layout(opt, 0, 0)
    # the reset prologue: 8 words per workgroup under the sharded image, 4 under the one-word image
    assert ctr_ints <= reset_ints == 256 * (4 if opt & ONE_WORD else 8)
    gn_lines = {_layout(opt, 0, s)[1] // LINE for s in range(SLOTS)}
    assert err // LINE not in gn_lines and err < ctr_ints
    for g in range(GROUPS):
        group_words = set()
        for s in range(SLOTS):
            im, gn, _, _, _ = _layout(opt, g, s)
            polled = _polled(im, False)
            assert im["sig"] in polled and set(polled) <= set(_polled(im, True))
            assert 0 <= min(polled) and max(_polled(im, True)) < ctr_ints and gn < ctr_ints
            group_words |= set(polled)
        assert not ({w // LINE for w in group_words} & (gn_lines | {err // LINE}))
        # the arrivals a wait for this group needs per hand-off: every slot of the group exactly once
        im = _layout(opt, g, 0)[0]
        signals = [_layout(opt, g, s)[0]["sig"] for s in range(SLOTS)]
        assert all(signals.count(w) == im["mul"] for w in group_words) and im["mul"] * len(group_words) == SLOTS


def test_targets_agree_for_every_reachable_handoff():
    top = 25 * 256 * 2  # 25 group hand-offs per evaluation, 256 steps, two evaluations a step
    for L in list(range(0, 60)) + [25 * 128 - 1, 25 * 128, 25 * 256 - 1, 25 * 256, top - 1, top]:
        shard, one = _layout(DEFAULT, 2, 9, L)[0], _layout(DEFAULT | ONE_WORD, 2, 9, L)[0]
        # "mul" is the library's per-word target at hand-off L: 8 L on each of 4 words against 32 L on one
        assert (shard["n"], one["n"]) == (4, 1)
        assert shard["mul"] == 8 * L and one["mul"] == 32 * L
        assert shard["n"] * shard["mul"] == one["mul"] < 2 ** 31
