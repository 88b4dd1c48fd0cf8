"""Helpers of dataset creation (reference: confignet/dataset_utils.py): the OpenFace output of a directory (`processed/<name>.csv`,
`processed/<name>_of_details.txt`), the similarity transform of the pre-normalisation and the CelebA attribute list.

OpenFace itself is neither bundled nor replaced: run_openface_on_dir runs the user's own FaceLandmarkImg build when `openface_path`
exists, and otherwise expects `processed/*.csv` next to the images together with the `landmarks_detected` marker file."""
import os
import subprocess

import numpy as np


def _headers(csv_file_path):
    with open(csv_file_path, "r") as fp:
        # OpenFace pads its column names with spaces
        return [header.strip() for header in fp.readline().split(",")]


def get_landmark_column_idxs_from_csv(csv_file_path, n_landmarks):
    headers = _headers(csv_file_path)
    names_2d = ["x_%d" % i for i in range(n_landmarks)] + ["y_%d" % i for i in range(n_landmarks)]
    names_3d = ["%s_%d" % (axis, i) for axis in "XYZ" for i in range(n_landmarks)]
    return [headers.index(n) for n in names_2d], [headers.index(n) for n in names_3d]


def get_pose_column_idxs_from_csv(csv_file_path):
    headers = _headers(csv_file_path)
    return [headers.index(n) for n in ("pose_Tx", "pose_Ty", "pose_Tz", "pose_Rx", "pose_Ry", "pose_Rz")]


def read_landmarks_and_pose_from_csv(csv_file_path, n_landmarks=68, confidence_threshold=0.6):
    """(landmarks (n, 2), landmarks_3d (n, 3), pose (6)) of the most confident face of the file, or
    (None, None, None) when its confidence is below the threshold.  The file holds all x, then all y (then all z): order='F'."""
    cols_2d, cols_3d = get_landmark_column_idxs_from_csv(csv_file_path, n_landmarks)
    cols = [_headers(csv_file_path).index("confidence")] + cols_2d + cols_3d + get_pose_column_idxs_from_csv(csv_file_path)
    table = np.loadtxt(csv_file_path, skiprows=1, usecols=cols, delimiter=",", ndmin=2)      # one row per detected face
    row = table[int(np.argmax(table[:, 0]))]
    if row[0] < confidence_threshold:
        return None, None, None
    n2, n3 = 1 + 2 * n_landmarks, 1 + 5 * n_landmarks
    landmarks = np.reshape(row[1:n2], (n_landmarks, 2), order="F")
    landmarks_3d = np.reshape(row[n2:n3], (n_landmarks, 3), order="F")
    return landmarks, landmarks_3d, row[n3:]


def read_estimated_intrinsics(details_file_path):
    """The camera matrix from the third line of `<name>_of_details.txt` ("...: fx, fy, cx, cy")."""
    with open(details_file_path, "r") as fp:
        lines = fp.readlines()
    fx, fy, cx, cy = [float(x) for x in lines[2].split(":")[1].split(",")][:4]
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return K


def get_similarity_transform(destination_landmarks, source_landmarks):
    """(T, t) with destination ~ T source + t in the least-squares sense, T = [[a, -b], [b, a]] (a rotation times a scale).  With
    the centred points read as complex numbers, a + ib = sum(conj(s) d) / sum(|s|^2)."""
    src_mean, dst_mean = source_landmarks.mean(axis=0), destination_landmarks.mean(axis=0)
    s, d = source_landmarks - src_mean, destination_landmarks - dst_mean
    energy = np.sum(s * s)
    a = np.sum(s * d) / energy
    b = np.sum(s[:, 0] * d[:, 1] - s[:, 1] * d[:, 0]) / energy
    T = np.array([[a, -b], [b, a]])
    return T, dst_mean - T @ src_mean


def parse_celeba_attribute_file(file_path):
    """list_attr_celeba.txt -> {picture name without extension: {attribute: 0 / 1}}.  The file's first line is a count, its second
    the attribute names, then one line per picture: its file name and a -1 / 1 per attribute."""
    with open(file_path, "r") as fp:
        rows = [line.split() for line in fp]
    names = rows[1]
    return {os.path.splitext(row[0])[0]: {n: int(v != "-1") for n, v in zip(names, row[1:])} for row in rows[2:] if row}


def run_openface_on_dir(input_dir, openface_path):
    """Landmarks for every picture of input_dir into input_dir/processed, once: the marker file `landmarks_detected` says that
    they are there (written by this function after a run, or by a user who supplies the CSV files).  The binary gets the reference's
    argument list; without a binary the reference's ImportError is raised and no marker is written."""
    marker = os.path.join(input_dir, "landmarks_detected")
    if os.path.exists(marker):
        return
    out_dir = os.path.join(input_dir, "processed")
    os.makedirs(out_dir, exist_ok=True)
    if openface_path is None or not os.path.exists(openface_path):
        raise ImportError("OpenFace not found, please download it using the download_deps.py script.")
    print("OpenFace landmark detection on %s" % input_dir)
    subprocess.call([openface_path, "-fdir", input_dir, "-wild", "-out_dir", out_dir, "-2Dfp", "-3Dfp", "-pose", "-multi_view 1"])
    open(marker, "w").close()
