"""The beam rule of FastGearDecoder.generate_beam restated in plain Python (lists and numpy float32 on the host), written from the
rule's text and independent of gear_amd/beam.py, the way sample_ref.py restates the sampler.

search() drives any pair  step(tokens: list[int]) -> logits [S, V] (a torch tensor)  /  reorder(idx: list[int]).

Rule.  Scores start at [0, -1e9, ...].  Per step: lp = log_softmax(fp32 logits), cand[b, t] = fp32(score[b] + lp[b, t]); the 2 S
largest candidates, equal values ordered by the lower flat index b V + t.  Walking them in order: a candidate whose token is EOS
finishes a hypothesis if its rank is < S (score cand / len ** length_penalty, len counting the prompt and the EOS) and is dropped
otherwise; the first S other candidates are the next beams.  reorder(beam indices), step(tokens).  Stop at max_length, or once at
least S hypotheses have finished and the S-th best finished score is >= the best live candidate / cur_len ** length_penalty.  At the
end the live beams join the finished ones with the same normalisation; best first, equal scores in the order they were added.
The normalisation is a double-precision division of the fp32 candidate value, rounded to fp32 when returned."""
import numpy as np
import torch


def _log_softmax(logits):
    return torch.log_softmax(logits.float(), -1).cpu().numpy()


def search(logits0, step, reorder, prompt, S, max_length, eos=None, length_penalty=1.0, n_return=1, pad=0):
    """-> dict(sequences [n][max_length], scores float32 [n], raw [n] (unnormalised sums), lengths [n], trace)
    trace: per step dict(beam_idx, tokens, finished=[(rank, beam)], boundary-free bookkeeping for the tests' conditions)."""
    hist = [list(prompt) for _ in range(S)]
    score = np.full(S, -1e9, np.float32)
    score[0] = 0.0
    done = []                      # (normalised, raw, tokens)
    trace = []
    logits = logits0
    length = len(prompt)
    while True:
        lp = _log_softmax(logits)
        V = lp.shape[1]
        cand = (score[:, None] + lp).astype(np.float32).reshape(-1)
        order = np.lexsort((np.arange(cand.size), -cand.astype(np.float64)))[:2 * S]
        length += 1
        beams, ended = [], []
        for rank, flat in enumerate(order):
            b, t = int(flat) // V, int(flat) % V
            value = float(cand[flat])
            if eos is not None and t == eos:
                if rank < S:
                    done.append((value / length ** length_penalty, value, hist[b] + [t]))
                    ended.append((rank, b))
                continue
            if len(beams) < S:
                beams.append((b, t, value))
        assert len(beams) == S
        hist = [hist[b] + [t] for b, t, _ in beams]
        score = np.array([v for _, _, v in beams], np.float32)
        trace.append(dict(beam_idx=[b for b, _, _ in beams], tokens=[t for _, t, _ in beams], finished=ended, length=length))
        if length >= max_length:
            break
        if len(done) >= S:
            kth = sorted((d[0] for d in done), reverse=True)[S - 1]
            if kth >= float(score[0]) / length ** length_penalty:
                break
        reorder([b for b, _, _ in beams])
        logits = step([t for _, t, _ in beams])
    for b in range(S):
        done.append((float(score[b]) / length ** length_penalty, float(score[b]), hist[b]))
    ranked = sorted(range(len(done)), key=lambda i: (-done[i][0], i))[:n_return]
    seqs = [done[i][2] + [pad] * (max_length - len(done[i][2])) for i in ranked]
    return dict(sequences=seqs, scores=np.array([done[i][0] for i in ranked], np.float32), raw=[done[i][1] for i in ranked],
                lengths=[len(done[i][2]) for i in ranked], trace=trace)
