"""SVM model files and file lists -- mirror of the part of ``sidekit/sv_utils.py`` the SVM back end uses: ``save_svm`` / ``read_svm``
(:51-73) and ``check_file_list`` (:76-91).  A model file is the reference's: a gzip stream that holds the pickle of the tuple ``(w, b)``,
so files written by either package are read by the other.  The ``initialize_iv_extraction_*`` functions are not built.  Host code only:
importing the module needs neither a GPU nor torch.
"""
import gzip
import os
import pickle

import numpy


def save_svm(svm_file_name, w, b):
    """Write the weights ``w`` and the bias ``b`` of one SVM; the directory is created when it is missing."""
    directory = os.path.dirname(svm_file_name)
    if directory and not os.path.exists(directory):
        os.makedirs(directory)
    with gzip.open(svm_file_name, "wb") as f:
        pickle.dump((w, b), f)


def read_svm(svm_file_name):
    """-> ``(w, b)`` of one SVM file, ``w`` without its axes of length 1"""
    with gzip.open(svm_file_name, "rb") as f:
        w, b = pickle.load(f)
    return numpy.squeeze(w), b


def check_file_list(input_file_list, file_name_structure):
    """The entries ``f`` of ``input_file_list`` (an array) for which the file ``file_name_structure.format(f)`` exists, and their indices:
    ``input_file_list[idx] == output_file_list``."""
    input_file_list = numpy.asarray(input_file_list)
    exists = numpy.array([os.path.isfile(file_name_structure.format(f)) for f in input_file_list], dtype=bool)
    output_file_list = input_file_list[exists]
    return output_file_list, numpy.flatnonzero(numpy.isin(input_file_list, output_file_list))
