"""The candidate stage of include/slamhip.h ("loop and relocalisation candidates") on another route: the loops of ORB-SLAM's
KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates over Python lists and ints, one query and one candidate
at a time.  Written from the header, not from csrc/loop_detect.hip and not from slamhip.loop_candidates_host."""

DERIVE = 0xFFFFFFFF


def candidates_ref(s, common, best, excluded, own, limit, min_s, mode):
    """One query.  s, common: lists [E]; best: list of E rows; excluded: list of ids (own included where the caller lists it);
    own: int; limit: int; min_s: int (DERIVE: from the excluded entries); mode: 0 loop, 1 relocalisation.
    -> dict(ids, scores, acc [E], gbest [E], skipped)."""
    E = len(s)
    skipped = 0
    connected = set()
    min_score = 0
    if mode == 0:
        derived = None
        for j in excluded:
            if j < 0 or j >= E:
                skipped += 1
                continue
            connected.add(j)
            if j != own and (derived is None or s[j] < derived):
                derived = s[j]
        min_score = min_s if min_s != DERIVE else (1 << 31 if derived is None else derived)
    # lKFsSharingWords and maxCommonWords
    sharing = []
    max_common = 0
    for i in range(E):
        if i in connected or i >= limit or common[i] <= 0:
            continue
        sharing.append(i)
        if common[i] > max_common:
            max_common = common[i]
    acc, gbest = [0] * E, [-1] * E
    out = dict(ids=[], scores=[], acc=acc, gbest=gbest, skipped=skipped)
    if not sharing:
        return out
    enough = set(i for i in sharing if 5 * common[i] > 4 * max_common)
    # lScoreAndMatch
    score_and_match = [i for i in sharing if i in enough and s[i] >= min_score]
    if not score_and_match:
        return out
    # lAccScoreAndMatch
    best_acc = 0
    for i in score_and_match:
        best_score, acc_score, best_kf = s[i], s[i], i
        for j in best[i]:
            if j < 0:
                continue
            if j >= E:
                out["skipped"] += 1
                continue
            if j in enough:
                acc_score += s[j]
                if s[j] > best_score:
                    best_kf, best_score = j, s[j]
        acc[i], gbest[i] = acc_score, best_kf
        if acc_score > best_acc:
            best_acc = acc_score
    already = set()
    for i in score_and_match:
        if 4 * acc[i] > 3 * best_acc:
            already.add(gbest[i])
    out["ids"] = sorted(already)
    out["scores"] = [s[i] for i in out["ids"]]
    return out

