"""Input files of the box-record converter's tests (tests/test_convert_boxes_cpu.py, tests/test_convert_boxes_gpu.py)."""


def annotation_xml(ident, persons, file_name=None):
    """the annotation of `<ident>.jpg`; persons: (type, xmin, ymin, xmax, ymax) each"""
    body = "".join("<person><bbox><type>%s</type><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bbox></person>"
                   % p for p in persons)
    return ("<annotation><file_name>%s</file_name>%s</annotation>" % (file_name or ident + ".jpg", body)).encode()
