"""`Logger`: the reference's TensorBoard logger (logger/logger.py) on `events.EventFileWriter`, minus its graph and
audio calls.

The reference registers summary ops on graph tensors, merges them into one `summary_op`, evaluates it in the step's
`session.run` and writes the result (trainer/mfcctrainer.py:266-297,310,343-357).  Here a summary is registered on a
SOURCE - whatever the trainer that owns the logger uses to name one of its tensors - and `merge_summary()` freezes the
registrations, in order, into `summary_op`: a list of (kind, tags, source).  The trainer evaluates it with
`summary(fetch)`: `fetch(kind, source)` returns

    "scalar"     a number
    "image"      uint8 [max_outputs, H, W, 3]: the images tf.summary.image would encode (ops.summary_images renders them)
    "histogram"  dict(min, max, num, sum, sum_squares, counts, limits) (ops.histogram_segments reduces them)

and the encoded values go to `write_summary(values, global_step)`.
"""
from . import events


def histogram_fields(name, counts, stats, nonfinite, limits):
    """one segment's outputs of ops.histogram_segments (counts [L], stats [4], nonfinite) -> the keyword arguments of
    `events.histogram_value`; a non-finite value raises, as TF's histogram summary op does"""
    if int(nonfinite):
        raise ValueError("Nan in summary histogram for: %s" % name)
    return dict(min=float(stats[0]), max=float(stats[1]), num=float(int(counts.sum())), sum=float(stats[2]),
                sum_squares=float(stats[3]), counts=counts, limits=limits)


class Logger(object):

    def __init__(self, log_dir, clock=None, hostname=None):
        self.log_dir = log_dir
        self.summary_op = None
        self._inputs = []
        kw = {} if clock is None else dict(clock=clock)
        self._writer = events.EventFileWriter(log_dir, hostname=hostname, **kw)

    @property
    def path(self):
        return self._writer.path

    def log_scalar(self, tag, value):
        self._inputs.append(("scalar", [events.sanitize_tag(tag)], value))

    def log_histogram(self, tag, value):
        self._inputs.append(("histogram", [events.sanitize_tag(tag)], value))

    def log_image(self, tag, value, max_outputs=1):
        """one output: tag `name/image`; more: `name/image/<i>`"""
        self._inputs.append(("image", events.image_tags(tag, max_outputs), value))

    def merge_summary(self):
        self.summary_op = list(self._inputs)

    def summary(self, fetch):
        """the encoded Summary.Values of `summary_op`, in registration order"""
        out = []
        for kind, tags, source in self.summary_op:
            got = fetch(kind, source)
            if kind == "scalar":
                out.append(events.scalar_value(tags[0], got))
            elif kind == "image":
                for tag, img in zip(tags, got):       # fewer images than max_outputs: a batch smaller than that
                    out.append(events.image_value(tag, img))
            else:
                out.append(events.histogram_value(tags[0], **got))
        return out

    def write_summary(self, values, global_step=None):
        self._writer.add_summary(values, 0 if global_step is None else int(global_step))

    def flush_writer(self):
        self._writer.flush()

    def close(self):
        self._writer.close()
