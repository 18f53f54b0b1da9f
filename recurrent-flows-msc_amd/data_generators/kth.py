"""KTH actions from local files, held on the device (the reference's data_generators/kth.py:10-68 as
RFN/trainer.py:141-153 drives it).

For each of the six classes `<data_root>/processed/<class>/{train,test}_meta<S>x<S>.t7` lists the videos of the split:
a Torch7 table of {vid = <directory>, files = {{<frame file>, ...}, ...}}, one entry of `files` per recorded sequence.
Channel 0 of every listed `processed/<class>/<vid>/<file>` is packed into a one-channel FrameStore (clips.py) once, or
loaded from a cache whose fingerprint (meta files and frames) matches; a batch is one launch of the clip-gather kernel.

Clip choice (kth.py:34-49 with addressed draws, clips.py): attempt a = 0, 1, ... draws class = randint(6) (draw 3a),
video = randint(n_videos[class]) (3a+1), sequence = randint(n_sequences[video]) (3a+2); the first attempt whose sequence
has at least seq_len frames is taken, with start = randint(0, length - seq_len + 1) (draw 3a+3: the last start
included, as random.randint).  len() is the reference's arbitrary len(os.listdir(processed)) * 36 * 5.

`read_t7` is a minimal reader of Torch7's binary serialisation (the reference uses the `torchfile` package): numbers,
strings, booleans, nil and plain tables.  It has only been checked against files written to the same description, not
against a real KTH meta file."""
import os
import struct

import numpy as np

from .clips import ClipDataset, draw_below, pack_or_load

CLASSES = ['boxing', 'handclapping', 'handwaving', 'jogging', 'running', 'walking']

_T7_NIL, _T7_NUMBER, _T7_STRING, _T7_TABLE, _T7_BOOLEAN = 0, 1, 2, 3, 5


class _T7(object):
    def __init__(self, raw):
        self.raw, self.pos, self.seen = raw, 0, {}

    def take(self, fmt, what):
        n = struct.calcsize(fmt)
        if self.pos + n > len(self.raw):
            raise ValueError("t7: truncated: %s (%d bytes) at byte offset %d of %d" % (what, n, self.pos, len(self.raw)))
        v = struct.unpack_from(fmt, self.raw, self.pos)[0]
        self.pos += n
        return v

    def obj(self):
        at = self.pos
        tag = self.take("<i", "a type tag")
        if tag == _T7_NIL:
            return None
        if tag == _T7_NUMBER:
            v = self.take("<d", "a number")
            return int(v) if v == v and abs(v) < 2 ** 53 and v == int(v) else v
        if tag == _T7_STRING:
            n = self.take("<i", "a string length")
            if n < 0:
                raise ValueError("t7: string length %d at byte offset %d" % (n, self.pos - 4))
            return self.take("<%ds" % n, "a string")
        if tag == _T7_BOOLEAN:
            return self.take("<i", "a boolean") != 0
        if tag == _T7_TABLE:
            ref = self.take("<i", "a table reference")
            if ref in self.seen:
                if self.seen[ref] is self:
                    raise ValueError("t7: table %d refers to itself (byte offset %d)" % (ref, at))
                return self.seen[ref]
            self.seen[ref] = self   # marks "being read"
            n = self.take("<i", "a table size")
            if n < 0:
                raise ValueError("t7: table size %d at byte offset %d" % (n, self.pos - 4))
            pairs = []
            for _ in range(n):
                k = self.obj()
                pairs.append((k, self.obj()))
            keys = [k for k, _ in pairs]
            if any(isinstance(k, (list, dict)) for k in keys):
                raise ValueError("t7: a table is used as a key in the table at byte offset %d" % at)
            if all(type(k) is int for k in keys) and sorted(keys) == list(range(1, n + 1)):
                table = [v for _, v in sorted(pairs, key=lambda kv: kv[0])]
            else:
                table = dict(pairs)
            self.seen[ref] = table
            return table
        raise ValueError("t7: unsupported type tag %d at byte offset %d" % (tag, at))


def read_t7(raw):
    """the object a Torch7 binary file (bytes, or a path) holds.  All values little-endian; an object is an int32 tag
    and a body: 0 nil; 1 number (float64; whole numbers come back as int); 2 string (int32 length, bytes -> bytes);
    3 table (int32 reference index; a seen index is that earlier table, else int32 pair count and count x (key, value));
    5 boolean (int32).  A table with keys exactly 1..n becomes a list, any other a dict (string keys are bytes).
    Any other tag -- 4, a torch class instance, included -- and truncated input raise ValueError naming the byte
    offset."""
    if not isinstance(raw, (bytes, bytearray, memoryview)):
        with open(raw, "rb") as f:
            raw = f.read()
    return _T7(bytes(raw)).obj()


def _decode_channel0(side):
    def decode(path):
        from PIL import Image   # only needed when frames are decoded: a matching cache never gets here
        with Image.open(path) as im:
            a = np.asarray(im.convert("RGB"))
        if a.shape[:2] != (side, side):
            raise ValueError("KTH: %s is %dx%d, expected %dx%d (frames are not resized)" %
                             (path, a.shape[0], a.shape[1], side, side))
        return a[:, :, :1]
    return decode


class KTH(ClipDataset):
    """The reference's KTH with its constructor arguments, plus `seed` (None = 0) keying the draws, `device` (where
    the frames live; default the current GPU), `cache` (a file prefix for the packed store), `length` (overrides the
    number of clips per epoch), `channels` (1, or 3 copies) and `store` (a ready FrameStore holding the sequences the
    meta files list, in their order: no frame is decoded)."""

    def __init__(self, train, data_root, seq_len=20, image_size=64, seed=None, device=None, cache=None, store=None,
                 length=None, channels=1):
        self.data_root = '%s/processed' % data_root
        self.image_size, self.classes = int(image_size), list(CLASSES)
        self.dirs = os.listdir(self.data_root)
        data_type = 'train' if train else 'test'
        metas, files, n_videos, n_sequences = [], [], [], []
        for c in self.classes:
            meta = '%s/%s/%s_meta%dx%d.t7' % (self.data_root, c, data_type, self.image_size, self.image_size)
            metas.append(meta)
            videos = read_t7(meta)
            if not isinstance(videos, list) or not videos:
                raise ValueError("KTH: %s lists no video" % meta)
            n_videos.append(len(videos))
            for vid in videos:
                seqs = vid.get(b'files') if isinstance(vid, dict) else None
                if not isinstance(vid.get(b'vid') if isinstance(vid, dict) else None, bytes) or \
                        not isinstance(seqs, list) or not seqs or \
                        not all(isinstance(s, list) and all(isinstance(f, bytes) for f in s) for s in seqs):
                    raise ValueError("KTH: %s: a video is not {vid = <name>, files = {{<file>, ...}, ...}}" % meta)
                n_sequences.append(len(seqs))
                dname = '%s/%s/%s' % (self.data_root, c, vid[b'vid'].decode())
                files += [['%s/%s' % (dname, f.decode()) for f in s] for s in seqs]
        # classes -> videos -> sequences, flattened in meta order
        self.n_videos = np.array(n_videos, dtype=np.int64)
        self.video0 = np.concatenate([[0], np.cumsum(self.n_videos)[:-1]]).astype(np.int64)
        self.n_sequences = np.array(n_sequences, dtype=np.int64)
        self.sequence0 = np.concatenate([[0], np.cumsum(self.n_sequences)[:-1]]).astype(np.int64)
        if store is None:
            store = pack_or_load(cache, str(data_root), files, _decode_channel0(self.image_size), self.image_size,
                                 self.image_size, 1, also=metas)
        if (store.H, store.W, store.Cs) != (self.image_size, self.image_size, 1):
            raise ValueError("KTH: the store holds %dx%dx%d frames, expected %dx%dx1" %
                             (store.H, store.W, store.Cs, self.image_size, self.image_size))
        if [int(n) for n in store.length] != [len(s) for s in files]:
            raise ValueError("KTH: the store's sequences are not the ones the %s meta files list" % data_type)
        if channels not in (1, 3):
            raise ValueError("KTH: 1 channel or 3 copies of it, got %r" % (channels,))
        self._setup(store, seq_len, channels, train, seed, device)
        if not (store.length >= self.seq_len).any():
            raise ValueError("KTH: no %s sequence under %s has %d frames" % (data_type, self.data_root, self.seq_len))
        self.length = len(self.dirs) * 36 * 5 if length is None else int(length)   # arbitrary, as the reference's

    def __len__(self):
        return self.length

    def epoch_choices(self, epoch):
        """(sequence, start frame) of every clip of an epoch, int64 [len(self)] each"""
        key, ids = (self.seed, self.split_id), self.sequence_ids(epoch)
        seq = np.zeros(len(self), dtype=np.int64)
        start = np.zeros(len(self), dtype=np.int64)
        todo = np.arange(len(self))
        a = 0
        while todo.size:
            s = ids[todo]
            c = draw_below(key, 3 * a, s, len(self.classes))
            v = self.video0[c] + draw_below(key, 3 * a + 1, s, self.n_videos[c])
            q = self.sequence0[v] + draw_below(key, 3 * a + 2, s, self.n_sequences[v])
            ok = self.store.length[q] >= self.seq_len
            seq[todo[ok]] = q[ok]
            start[todo[ok]] = draw_below(key, 3 * a + 3, s[ok], self.store.length[q[ok]] - self.seq_len + 1)
            todo = todo[~ok]
            a += 1
        return seq, start

    def _epoch_first(self, epoch):
        seq, start = self.epoch_choices(epoch)
        return np.ascontiguousarray(self.store.offset[seq] + start, dtype=np.int64)
