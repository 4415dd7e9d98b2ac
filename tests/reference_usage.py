"""Inputs shared by tests/test_reference_scripts.py and the script that records its
golden file (tests/golden/make_golden_refscripts.py)."""
import numpy as np


def tiny_nmf_inputs(ds):
    """(train matrix, [user, item] test rows, users, items) of the NMF comparison."""
    import scipy.sparse as sp
    U, I = ds["user_num"], ds["item_num"]
    mat = sp.dok_matrix((U, I), dtype=np.float32)
    for u, i in zip(ds["train_users"], ds["train_items"]):
        mat[int(u), int(i)] = 1.0
    test = []
    for u, p, negs in zip(ds["test_users"], ds["test_items"], ds["test_negatives"]):
        test.append([int(u), int(p)])
        test += [[int(u), int(n)] for n in negs]
    return mat, test, np.array([0, 3, U - 1, U + 5]), np.array([1, 0, I - 1, 2])
