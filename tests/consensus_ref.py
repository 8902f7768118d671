"""The definition of the consensus choice inside an n-best list, in plain Python ints and float64 (paraformer_hip.h "Consensus
choice and token confidence"; csrc/k_consensus.hip and pf_host_consensus are held to it bit for bit).

A list is N hypotheses (1 <= N <= 64) of 0 .. 255 int32 ids, compared on all 32 bits, with weights p_i >= 0 (finite float64).
  posterior  p_i = exp(scale (s_i - max s)) / sum_k exp(scale (s_k - max s)), the sum over k ascending, scale > 0
  distance   D[i][j] = Levenshtein distance of the id sequences, unit costs
  risk       risk_i = sum_j p_j D[i][j], j ascending, each product rounded to float64, then added
  winner     the smallest i of minimal risk (strict < scanning upward)
  alignment  of y = h_j to x = h_w: E[0][b] = b, E[a][0] = a, E[a][b] = min(E[a-1][b-1] + (x_a != y_b), E[a-1][b] + 1,
             E[a][b-1] + 1); back from (n_w, n_j): if the diagonal term gives E[a][b] step diagonally and m_j[a-1] = (x_a == y_b),
             else if the up term does step up and m_j[a-1] = 0, else step left; on a border the step is forced (up: m_j[a-1] = 0)
  confidence conf[t] = sum_j p_j m_j[t], j ascending, t < n_w
"""
import math


def posterior(scores, scale=1.0):
    top = max(scores)
    e = [math.exp(scale * (s - top)) for s in scores]
    total = 0.0
    for x in e:
        total += x
    return [x / total for x in e]


def table(x, y):
    E = [[0] * (len(y) + 1) for _ in range(len(x) + 1)]
    E[0] = list(range(len(y) + 1))
    for a in range(1, len(x) + 1):
        E[a][0] = a
        for b in range(1, len(y) + 1):
            E[a][b] = min(E[a - 1][b - 1] + (x[a - 1] != y[b - 1]), E[a - 1][b] + 1, E[a][b - 1] + 1)
    return E


def match_mask(x, y):
    """m[t] = 1 where the canonical alignment of y to x pairs x[t] with an equal id"""
    E, m = table(x, y), [0] * len(x)
    a, b = len(x), len(y)
    while a > 0 and b > 0:
        if E[a][b] == E[a - 1][b - 1] + (x[a - 1] != y[b - 1]):
            m[a - 1] = int(x[a - 1] == y[b - 1])
            a, b = a - 1, b - 1
        elif E[a][b] == E[a - 1][b] + 1:
            a -= 1
        else:
            b -= 1
    return m


def consensus(hyps, p):
    """(winner, risk [N], conf [n_winner], D [N][N]) of one list"""
    n = len(hyps)
    D = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            D[i][j] = D[j][i] = table(hyps[i], hyps[j])[-1][-1]
    risk = []
    for i in range(n):
        r = 0.0
        for j in range(n):
            r = r + p[j] * D[i][j]
        risk.append(r)
    w = 0
    for i in range(n):
        if risk[i] < risk[w]:
            w = i
    conf = [0.0] * len(hyps[w])
    for j in range(n):
        m = match_mask(hyps[w], hyps[j])
        for t in range(len(conf)):
            conf[t] = conf[t] + p[j] * m[t]
    return w, risk, conf, D
