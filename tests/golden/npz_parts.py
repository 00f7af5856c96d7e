"""Fixtures as .npz files of at most PART_BYTES each.

A fixture `name` is either one file name.npz or, where that would be larger, the files name.part0.npz,
name.part1.npz, ...: each holds some of the arrays whole, and together they hold every key once.
load(dir, name) returns the same dict either way; save(dir, name, arrays) writes whichever form fits.
"""
import glob
import io
import os

import numpy as np

PART_BYTES = 1000000        # under the 1 MiB limit for a committed file


def _paths(directory, name):
    one = os.path.join(directory, name + '.npz')
    if os.path.exists(one):
        return [one]
    return sorted(glob.glob(os.path.join(glob.escape(directory), glob.escape(name) + '.part[0-9]*.npz')))


def load(directory, name):
    paths = _paths(directory, name)
    if not paths:
        raise FileNotFoundError('no fixture %s(.part*).npz in %s' % (name, directory))
    out = {}
    for p in paths:
        with np.load(p, allow_pickle=False) as z:
            for k in z.files:
                if k in out:
                    raise ValueError('fixture %s: key %s in more than one part' % (name, k))
                out[k] = z[k]
    return out


def _packed_size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getbuffer().nbytes


def save(directory, name, arrays):
    """Write the fixture and return the paths written.  Arrays go into parts in key order, first fit."""
    for p in _paths(directory, name):
        os.remove(p)
    if _packed_size(arrays) <= PART_BYTES:
        paths = [os.path.join(directory, name + '.npz')]
        np.savez_compressed(paths[0], **arrays)
        return paths
    parts = []
    for k, v in arrays.items():
        for part in parts:
            if _packed_size(dict(part, **{k: v})) <= PART_BYTES:
                part[k] = v
                break
        else:
            if _packed_size({k: v}) > PART_BYTES:
                raise ValueError('fixture %s: array %s alone is above %d bytes packed' % (name, k, PART_BYTES))
            parts.append({k: v})
    paths = [os.path.join(directory, '%s.part%d.npz' % (name, i)) for i in range(len(parts))]
    for p, part in zip(paths, parts):
        np.savez_compressed(p, **part)
    return paths
